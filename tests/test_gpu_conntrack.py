"""GPU: the connection table on the device (neb_conntrack_*, conntrack.hip) against its host form and
the model (tests/conntrack_ref.py) on the directed cases and on random scripts, with every output
pre-filled to show that nothing else is written; what one stream's calls see of each other; copies of
a key in one batch; full tables; compaction; lookups beside adds and evicts on another stream; and the
call in its two places: between a real receive's inner resolve and the coalescer, and between the TX
resolve and the seal."""
import ctypes as C
import random

import numpy as np
import pytest

import conntrack_cases as K
import conntrack_ref as R
from nebula_amd import _lib as L
from nebula_amd import firewall as F
from nebula_amd.inside import TX_PACKET_DTYPE

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257]
PLAIN, FW, WORK = L.PLAIN_PACKET_DTYPE.itemsize, L.FW_PACKET_DTYPE.itemsize, L.CT_WORK_DTYPE.itemsize


def _dev(engine):
    import torch

    return torch.device("cuda", engine.device)


def _up(engine, a, skew=0):
    """The bytes of `a` on the device, `skew` bytes past an allocation's (256-byte aligned) base."""
    import torch

    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    d = torch.empty(len(b) + skew, dtype=torch.uint8, device=_dev(engine))
    d[skew:] = torch.from_numpy(b.copy()).to(_dev(engine))
    return d[skew:]


def _fill(engine, count, value, dtype):
    import torch

    return torch.full((count,), value, dtype=dtype, device=_dev(engine))


class DeviceRunner:
    """conntrack_ref.play's steps on a device table. Every output has a guard behind it, pre-filled
    like the output itself (0xEE bytes, -7 words); d_fw and d_keys sit at their 16-byte alignment only."""
    exact = False  # which copy of a key answers NEW, and which copy of an evicted one 0, is the device's choice

    def __init__(self, engine, ct):
        self.engine, self.ct = engine, ct

    def lookup(self, fw, status, now, hold, work_cap):
        import torch

        e, n = self.engine, len(fw)
        cap = n if work_cap is None else work_cap
        d_fw = _up(e, fw, skew=16)
        d_st = _up(e, np.array(status, np.int32)).view(torch.int32)
        d_verdict, d_work = _fill(e, n + 16, 0xEE, torch.uint8), _fill(e, (cap + 1) * WORK, 0xEE, torch.uint8)
        d_counts = _fill(e, 8, -7, torch.int32)
        plain0 = tx0 = d_plain = d_tx = None
        if hold == "rx":
            plain0 = np.zeros(n, L.PLAIN_PACKET_DTYPE)
            plain0["flags"], plain0["off"], plain0["len"] = L.PLAIN_PARSED, np.arange(n) * 64, 60
            d_plain = _up(e, plain0)
        if hold == "tx":
            tx0 = np.zeros(n, TX_PACKET_DTYPE)
            tx0["tunnel"], tx0["len"] = np.arange(n), 99
            d_tx = _up(e, tx0)
        self.ct.lookup_device(d_fw, d_st, n, now, d_verdict, d_counts, d_plain, d_tx, d_work, cap)
        torch.cuda.synchronize()
        verdict, counts = d_verdict.cpu().numpy(), d_counts.cpu().numpy()
        assert (verdict[n:] == 0xEE).all() and (counts[4:] == -7).all()
        counts = counts[:4].view(np.uint32)
        nw = min(int(counts[3]), cap)
        work = d_work.cpu().numpy()
        assert (work[nw * WORK:] == 0xEE).all()  # entries past the count, and past the cap, are not written
        plain = tx = None
        if hold == "rx":
            raw, raw0 = d_plain.cpu().numpy().reshape(n, PLAIN), plain0.view(np.uint8).reshape(n, PLAIN)
            assert (raw[:, :31] == raw0[:, :31]).all()  # the flags byte and nothing else
            plain = raw.reshape(-1).view(L.PLAIN_PACKET_DTYPE)
        if hold == "tx":
            raw, raw0 = d_tx.cpu().numpy().reshape(n, 32), tx0.view(np.uint8).reshape(n, 32)
            assert (raw[:, :12] == raw0[:, :12]).all() and (raw[:, 16:] == raw0[:, 16:]).all()  # the tunnel and nothing else
            tx = raw.reshape(-1).view(TX_PACKET_DTYPE)
        assert d_fw.cpu().numpy().tobytes() == fw.tobytes()
        return verdict[:n], work[:nw * WORK].view(L.CT_WORK_DTYPE), counts, d_st.cpu().numpy(), plain, tx

    def add(self, fw, incoming, now):
        import torch

        e, n = self.engine, len(fw)
        d_res = _fill(e, (n + 1) * 8, 0xEE, torch.uint8)
        self.ct.add_device(_up(e, fw, skew=16), _up(e, np.array(incoming, np.uint8)), n, now, d_res)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy()
        assert (res[n * 8:] == 0xEE).all()
        return res[:n * 8].view(L.CT_RESULT_DTYPE)

    def evict(self, fw, now, force):
        import torch

        e, n = self.engine, len(fw)
        d_rem = _fill(e, n + 1, -7, torch.int64)
        self.ct.evict_device(_up(e, fw, skew=16), n, now, d_rem, force)
        torch.cuda.synchronize()
        rem = d_rem.cpu().numpy()
        assert rem[n] == -7
        return rem[:n]


DEVICE_CASES = [c for c in K.all_cases() if c.device]


@pytest.mark.parametrize("case", DEVICE_CASES, ids=[c.name for c in DEVICE_CASES])
def test_directed_case_device_equals_host_equals_model(engine, case):
    """The model stands between the two: the host form plays the same scripts against it in
    test_conntrack_cases.py. Here also the images' entries are compared (which of two colliding keys
    of one batch sits first in their chain is the device's choice, so not the slots)."""
    with F.Conntrack(engine, case.capacity, seed=K.SEED, max_batch=case.max_batch) as ct, \
            F.Conntrack(None, case.capacity, seed=K.SEED, max_batch=case.max_batch) as host:
        model = R.Model(case.capacity)
        R.play(case.steps, model, DeviceRunner(engine, ct))
        case.reached(ct)
        R.play(case.steps, R.Model(case.capacity), R.HostRunner(host))
        assert R.table_snapshot(ct) == R.table_snapshot(host) and ct.count() == host.count()
        d, h = ct.dump(), host.dump()
        assert ((d["state"] == 0) == (h["state"] == 0)).all()  # the same slots in use, whoever sits where
        # compaction, then every lookup of the case again, on the entries the case left
        R.play([("compact",)] + [st for st in case.steps if st[0] == "lookup"], model, DeviceRunner(engine, ct))


@pytest.mark.parametrize("capacity", [1, 4, 1024])
def test_random_scripts_device_equals_model(engine, capacity):
    rng = np.random.default_rng(100 + capacity)
    keys = K.universe(capacity)  # as many keys as places: which key a full table refuses is unspecified
    with F.Conntrack(engine, capacity, seed=K.SEED + capacity, max_batch=257) as ct:
        model = R.Model(capacity)
        K.random_script(rng, model, DeviceRunner(engine, ct), keys, 40, SIZES)
        # compaction, then the earlier assertions again
        R.play([("compact",)], model, DeviceRunner(engine, ct))
        K.random_script(rng, model, DeviceRunner(engine, ct), keys, 10, SIZES)


def _lookup(engine, ct, d_fw, n, now, stream=None):
    import torch

    d_st = torch.zeros(n, dtype=torch.int32, device=_dev(engine))
    d_v, d_c = _fill(engine, n, 0xEE, torch.uint8), _fill(engine, 4, -7, torch.int32)
    ct.lookup_device(d_fw, d_st, n, now, d_v, d_c, stream=stream)
    return d_v, d_c


def _churn_and_compact(engine, ct):
    """Leaves `ct` a compacted table: flows come and go (tombstones in the chains), then the switch."""
    junk = F.fw_packets([("172.16.0.1", f"172.16.{i >> 8}.{i & 255}", 7, 9, 17) for i in range(200)])
    run = DeviceRunner(engine, ct)
    assert (run.add(junk, [0] * 200, 1)["code"] == L.CT_NEW).all()
    assert (run.evict(junk, 1, True) == 0).all() and ct.count()[:2] == (0, 200)
    ct.compact()
    assert ct.count()[:2] == (0, 0) and not ct.dump()["state"].any()


@pytest.mark.parametrize("compacted", [False, True], ids=["fresh", "compacted"])
def test_one_stream_orders_the_calls_without_a_host_sync(engine, compacted):
    import torch

    keys = K.universe(300)
    n = len(keys)
    with F.Conntrack(engine, 512, seed=1, max_batch=512) as ct:
        if compacted:
            _churn_and_compact(engine, ct)
        d_keys = _up(engine, keys)
        d_res = _fill(engine, n * 8, 0xEE, torch.uint8)
        d_rem = _fill(engine, n, -7, torch.int64)
        # add, then lookup: no host sync between
        ct.add_device(d_keys, _up(engine, np.ones(n, np.uint8)), n, K.T0, d_res)
        v1, c1 = _lookup(engine, ct, d_keys, n, K.T0 + 1000)
        # lookup twice in a row: the second, with an earlier clock, sees the first's refresh and keeps it
        v2, c2 = _lookup(engine, ct, d_keys, n, K.T0 + 10)
        ct.evict_device(d_keys, n, K.T0 + 2000, d_rem)
        v3, c3 = _lookup(engine, ct, d_keys, n, K.T0 + 3000)
        ct.evict_device(d_keys[:FW * 100], 100, K.T0, d_rem[:100], force=True)
        v4, c4 = _lookup(engine, ct, d_keys, n, K.T0 + 3000)
        torch.cuda.synchronize()
        assert (d_res.cpu().numpy().view(L.CT_RESULT_DTYPE)["code"] == L.CT_NEW).all()
        for v, c in ((v1, c1), (v2, c2), (v3, c3)):
            assert (v.cpu().numpy() == L.CT_HIT).all() and c.cpu().numpy().tolist() == [n, 0, 0, 0]
        timeout = np.array([R.Model(1).timeout(k) for k in R.keys_of(keys)], np.int64)
        rem = d_rem.cpu().numpy()
        assert (rem[100:] == K.T0 + 1000 + timeout[100:] - (K.T0 + 2000)).all()  # the first lookup's Expires
        assert (rem[:100] == 0).all()
        assert v4.cpu().numpy().tolist() == [L.CT_MISS] * 100 + [L.CT_HIT] * 200 and c4.cpu().numpy().tolist() == [200, 100, 0, 100]
        assert ct.count() == (200, 100, 1024)
        e = ct.entries()
        assert all(e[k][0] == K.T0 + 3000 + t for k, t in list(zip(R.keys_of(keys), timeout))[100:])


@pytest.mark.parametrize("compacted", [False, True], ids=["fresh", "compacted"])
def test_duplicate_key_add_batches(engine, compacted):
    rng = np.random.default_rng(5)
    keys = K.universe(100)
    with F.Conntrack(engine, 256, seed=2, max_batch=8192) as ct:
        if compacted:
            _churn_and_compact(engine, ct)
        first = DeviceRunner(engine, ct).add(keys[:20], [0] * 20, K.T0)
        assert (first["code"] == L.CT_NEW).all() and ct.count()[0] == 20
        pick = rng.integers(0, 100, 8192)
        inc = rng.integers(0, 2, 8192).astype(np.uint8)
        res = DeviceRunner(engine, ct).add(keys[pick], inc, K.T0 + 1)
        assert ct.count()[0] == 100  # rose by the number of distinct new keys
        e = ct.entries()
        assert len(e) == 100  # each once
        all_keys = R.keys_of(keys)
        for j in range(100):
            idx = np.flatnonzero(pick == j)
            codes = sorted(res["code"][idx].tolist())
            assert codes == [L.CT_EXISTING if j < 20 else L.CT_NEW] + [L.CT_DUP] * (len(idx) - 1)
            assert len(set(res["slot"][idx].tolist())) == 1 and e[all_keys[j]][3] == res["slot"][idx[0]]
            assert e[all_keys[j]][1] == inc[idx[-1]]  # the last copy's
            assert e[all_keys[j]][0] == K.T0 + 1 + R.Model(1).timeout(all_keys[j])


def test_full_table_batches(engine):
    keys = K.universe(500)
    with F.Conntrack(engine, 300, seed=3, max_batch=1024) as ct:
        run = DeviceRunner(engine, ct)
        res = run.add(keys, [1] * 500, K.T0)
        codes = res["code"]
        assert sorted(set(codes.tolist())) == [L.CT_NEW, L.CT_FULL] and (codes == L.CT_NEW).sum() == 300
        live, tombs, slots = ct.count()
        # live == capacity; a refused key that had taken a slot on its way in left it a tombstone
        assert (live, slots) == (300, 1024) and tombs <= 200
        v, work, counts, *_ = run.lookup(keys, [0] * 500, K.T0 + 1, None, None)
        assert (v == np.where(codes == L.CT_NEW, L.CT_HIT, L.CT_MISS)).all()  # refused keys MISS
        assert counts.tolist() == [300, 200, 0, 200] and work["packet"].tolist() == np.flatnonzero(codes == L.CT_FULL).tolist()
        again = run.add(keys, [0] * 500, K.T0 + 2)["code"]  # full: the tracked ones are overwritten, no other gets in
        assert (again == np.where(codes == L.CT_NEW, L.CT_EXISTING, L.CT_FULL)).all()
        assert ct.count() == (300, tombs, 1024)  # and a full table is left as it is
        # room for 100: exactly 100 of the refused get in
        gone = np.flatnonzero(codes == L.CT_NEW)[:100]
        assert (run.evict(keys[gone], K.T0, True) == 0).all() and ct.count() == (200, tombs + 100, 1024)
        refused = np.flatnonzero(codes == L.CT_FULL)
        third = run.add(keys[refused], [0] * len(refused), K.T0 + 3)["code"]
        assert (third == L.CT_NEW).sum() == 100 and (third == L.CT_FULL).sum() == len(refused) - 100
        assert ct.count()[0] == 300
        before = {k: v[:3] for k, v in ct.entries().items()}
        ct.compact()
        assert ct.count() == (300, 0, 1024) and {k: v[:3] for k, v in ct.entries().items()} == before
        v2 = run.lookup(keys, [0] * 500, K.T0 + 1, None, 0)[0]
        assert (v2 == L.CT_HIT).sum() == 300


def _add_over_capacity(engine, ct, keys, pick, inc, now):
    """One add of keys[pick] that may cross the table's capacity. Which keys are refused is the
    device's choice; everything else is fixed: all copies of a key agree (one NEW or EXISTING and
    DUPs with one slot, or FULL throughout), keys that were in the table stay, exactly
    min(capacity, live + distinct new keys) entries are live, the admitted entries hold the last
    copy's incoming, and a lookup HITs the admitted keys and MISSes the refused ones.
    Returns the set of refused key indexes."""
    run = DeviceRunner(engine, ct)
    all_keys = R.keys_of(keys)
    before = ct.entries()
    res = run.add(keys[pick], inc, now)
    after = ct.entries()
    refused, fresh = set(), 0
    for j in sorted(set(pick.tolist())):
        idx = np.flatnonzero(pick == j)
        codes = sorted(res["code"][idx].tolist())
        if codes[0] == L.CT_FULL:
            assert codes == [L.CT_FULL] * len(idx), (j, codes)  # as do all copies of its key
            assert (res["slot"][idx] == L.CT_NO_SLOT).all() and all_keys[j] not in before and all_keys[j] not in after
            refused.add(j)
            continue
        was = all_keys[j] in before
        assert codes == [L.CT_EXISTING if was else L.CT_NEW] + [L.CT_DUP] * (len(idx) - 1), (j, codes)
        fresh += not was
        entry = after[all_keys[j]]
        assert set(res["slot"][idx].tolist()) == {entry[3]}
        assert entry[:3] == (now + R.Model(1).timeout(all_keys[j]), int(inc[idx[-1]]), 0)  # the last copy's incoming
    distinct_new = len({all_keys[j] for j in set(pick.tolist())} - set(before))
    assert len(after) == ct.count()[0] == min(ct.capacity, len(before) + distinct_new)  # exactly capacity when it overflows
    assert fresh == len(after) - len(before) and set(before) <= set(after)
    order = np.array(sorted(set(pick.tolist())))
    v = run.lookup(keys[order], [0] * len(order), now, None, 0)[0]
    assert v.tolist() == [L.CT_MISS if j in refused else L.CT_HIT for j in order]
    return refused


@pytest.mark.parametrize("capacity,nkeys,n", [(4, 6, 6), (4, 6, 384), (1, 2, 256), (64, 200, 4096), (300, 500, 8192)])
def test_copies_of_new_keys_in_the_batch_that_fills_the_table(engine, capacity, nkeys, n):
    """Duplicate keys together with FULL: the claimers of the last places and the copies that find
    the table full race in one launch. (4, 6, 6) is the directed case 'FULL by capacity', whose
    script fixes which keys are refused and so plays on the host form only."""
    keys = K.universe(nkeys)
    for seed in range(6):
        rng = np.random.default_rng(1000 * capacity + seed)
        with F.Conntrack(engine, capacity, seed=K.SEED + seed, max_batch=8192) as ct:
            pick = rng.permutation(np.arange(n) % nkeys) if seed % 2 else np.repeat(np.arange(nkeys), n // nkeys)
            inc = rng.integers(0, 2, len(pick)).astype(np.uint8)
            refused = _add_over_capacity(engine, ct, keys, pick, inc, K.T0)
            assert len(refused) == nkeys - capacity
            # the table is full: the same batch again renews what is there, and is otherwise left as it is
            tombs = ct.count()[1]
            assert _add_over_capacity(engine, ct, keys, pick, inc, K.T0 + 1) == refused and ct.count()[1] == tombs
            # one place free, many copies of the refused keys after it: one key gets it, whole
            gone = next(j for j in range(nkeys) if j not in refused)
            assert DeviceRunner(engine, ct).evict(keys[gone:gone + 1], K.T0, True).tolist() == [0]
            if ct.count()[1] >= ct.slots - ct.capacity:
                ct.compact()
            again = np.array([j for j in pick.tolist() if j in refused])
            left = _add_over_capacity(engine, ct, keys, again, inc[:len(again)], K.T0 + 2)
            assert len(left) == len(refused) - 1


def test_lookups_beside_adds_and_evicts_on_another_stream(engine):
    """A steady key never misses while another stream adds and evicts around it."""
    import torch

    steady, churn = K.universe(256), K.universe(1024)[256:]
    with F.Conntrack(engine, 1024, seed=4, max_batch=1024) as ct:
        d_steady, d_churn = _up(engine, steady), _up(engine, churn)
        n, m = len(steady), len(churn)
        d_res, d_rem = _fill(engine, m * 8, 0, torch.uint8), _fill(engine, m, -7, torch.int64)
        d_inc = _up(engine, np.zeros(m, np.uint8))
        ct.add_device(d_steady, d_inc[:n], n, K.T0, d_res[:n * 8])
        torch.cuda.synchronize()
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        outs = []
        for r in range(12):
            ct.add_device(d_churn, d_inc, m, K.T0 + r, d_res, stream=sa.cuda_stream)
            outs.append(_lookup(engine, ct, d_steady, n, K.T0 + r, stream=sb.cuda_stream))
            ct.evict_device(d_churn, m, K.T0 + r, d_rem, force=True, stream=sa.cuda_stream)
            outs.append(_lookup(engine, ct, d_steady, n, K.T0 + r, stream=sb.cuda_stream))
            if r % 4 == 3:  # tombstones: compact, with nothing else running
                torch.cuda.synchronize()
                ct.compact(stream=sa.cuda_stream)
        torch.cuda.synchronize()
        for v, c in outs:
            assert (v.cpu().numpy() == L.CT_HIT).all() and c.cpu().numpy().tolist() == [n, 0, 0, 0]
        assert ct.count()[0] == n


def test_argument_checks(engine):
    import torch

    lib = L.lib()
    keys = K.universe(8)
    with F.Conntrack(engine, 4, max_batch=4) as ct, F.Conntrack(None, 4, max_batch=4) as host:
        d_fw = _up(engine, keys, skew=16)
        d_st = torch.zeros(8, dtype=torch.int32, device=_dev(engine))
        d_v, d_c = _fill(engine, 8, 0xEE, torch.uint8), _fill(engine, 4, -7, torch.int32)
        d_work, d_plain = _fill(engine, 8 * WORK + 16, 0xEE, torch.uint8), _fill(engine, 8 * PLAIN + 16, 0xEE, torch.uint8)
        d_res, d_rem = _fill(engine, 64, 0xEE, torch.uint8), _fill(engine, 8, -7, torch.int64)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        e, h, s = engine.handle, ct.handle, C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def look(table=h, eng=e, fw=d_fw, n=4, work=d_work, plain=None, counts=d_c):
            return lib.neb_conntrack_lookup_batch(eng, table, p(fw), p(d_st), n, 0, p(d_v), p(plain) if plain is not None else None,
                                                  None, p(work), 4, p(counts) if counts is not None else None, s)
        assert look(n=5) == L.ERR_INVALID  # n > max_batch
        assert look(fw=d_fw[8:]) == L.ERR_INVALID and look(work=d_work[8:]) == L.ERR_INVALID  # misaligned
        assert look(plain=d_plain[8:]) == L.ERR_INVALID
        assert look(table=host.handle) == L.ERR_INVALID and look(eng=None) == L.ERR_INVALID  # host-only table; no engine
        assert look(counts=None) == L.ERR_INVALID
        assert lib.neb_conntrack_add_batch(e, h, p(d_fw), p(d_v), 5, 0, p(d_res), s) == L.ERR_INVALID
        assert lib.neb_conntrack_add_batch(e, h, p(d_fw[8:]), p(d_v), 4, 0, p(d_res), s) == L.ERR_INVALID
        assert lib.neb_conntrack_add_batch(e, host.handle, p(d_fw), p(d_v), 4, 0, p(d_res), s) == L.ERR_INVALID
        assert lib.neb_conntrack_evict_batch(e, h, p(d_fw), 5, 0, 0, p(d_rem), s) == L.ERR_INVALID
        assert lib.neb_conntrack_evict_batch(e, h, p(d_fw[8:]), 4, 0, 0, p(d_rem), s) == L.ERR_INVALID
        assert lib.neb_conntrack_evict_batch(e, host.handle, p(d_fw), 4, 0, 0, p(d_rem), s) == L.ERR_INVALID
        # a device table has no host form
        st = np.zeros(4, np.int32)
        with pytest.raises(L.NebError):
            ct.lookup_host(keys[:4], st, 0)
        # n == 0: NEB_OK, nothing enqueued
        assert look(n=0) == L.OK
        assert lib.neb_conntrack_add_batch(e, h, None, None, 0, 0, None, s) == L.OK
        assert lib.neb_conntrack_evict_batch(e, h, None, 0, 0, 0, None, s) == L.OK
        torch.cuda.synchronize()
        for t in (d_v, d_work, d_plain, d_res):
            assert (t.cpu().numpy() == 0xEE).all()  # nothing launched, nothing written
        assert (d_c.cpu().numpy() == -7).all() and (d_rem.cpu().numpy() == -7).all() and ct.count()[0] == 0
        assert look() == L.OK  # and the call as the refused ones meant it goes through
        torch.cuda.synchronize()
        assert d_v.cpu().numpy()[:4].tolist() == [L.CT_MISS] * 4 and d_c.cpu().numpy().tolist() == [0, 4, 0, 4]


# ---- in its place on the RX side: real receive -> inner resolve -> lookup -> coalescer -----------------

def test_between_the_inner_resolve_and_the_coalescer(engine, oracle_mod):
    import torch

    import relay_forward_ref as RF
    import rx_inner_cases as RC
    from nebula_amd import outside as O
    from nebula_amd.connection_state import Bits, DeviceWindows, rx_open_wire_batch_device
    from nebula_amd.hostmap import PeerTable, routable
    from nebula_amd.noiseutil import CipherAESGCM
    from test_gpu_rx_inner import _traffic

    alg, ntun = L.ALG_AESGCM, 3
    rng = random.Random(77)
    keys = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(ntun)]
    ciphers = [CipherAESGCM.Cipher(engine, k) for k in keys]
    dw = None
    try:
        traffic = _traffic(rng, ntun, 300)
        ctr = [10] * ntun
        arena, pk = bytearray(b"\0" * 3), []
        for t, p, (typ, sub), forged, _, _ in traffic:
            ctr[t] += 1
            wire = bytearray(RF.seal_message(oracle_mod, alg, keys[t], 0x100 + t, ctr[t], p, typ, sub))
            if forged:
                wire[-1] ^= 1
            pk.append((len(arena), len(wire), ciphers[t].key_id))
            arena += wire + b"\0" * (len(pk) % 4)
        n = len(pk)
        pkt = np.array(pk, L.RX_PACKET_DTYPE)
        epoch = np.zeros(max(c.key_id for c in ciphers) + 1, np.uint64)
        for t in range(ntun):
            epoch[ciphers[t].key_id] = 40 + t
        tunnel_of = np.array([t for t, *_ in traffic])
        cap = int(((pkt["len"].astype(np.int64) + 15) & ~15).sum())
        dev = _dev(engine)

        def receive(ct, now):
            """open -> inner resolve -> [lookup with hold] -> coalesce, on one stream -> what the TUN gets."""
            nonlocal dw
            dw = DeviceWindows(engine, engine.max_keys, 1024)
            for c in ciphers:
                w = Bits(1024)
                dw.load(c.key_id, w)
                w.destroy()
            d_pk, d_arena = _up(engine, pkt), _up(engine, np.frombuffer(bytes(arena), np.uint8))
            d_st = _fill(engine, n, -1, torch.int32)
            d_plain, d_fw, d_in = _fill(engine, n * PLAIN, 0xEE, torch.uint8), _fill(engine, n * FW, 0xEE, torch.uint8), \
                _fill(engine, n, -7, torch.int32)
            d_out = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
            d_writes = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
            d_nw, d_pw, d_ps = (torch.zeros(k, dtype=torch.int32, device=dev) for k in (1, n, n))
            d_v, d_c, d_work = _fill(engine, n, 0xEE, torch.uint8), _fill(engine, 4, -7, torch.int32), \
                _fill(engine, n * WORK, 0xEE, torch.uint8)
            rx_open_wire_batch_device(engine, alg, dw, d_pk, d_arena, d_st, L.KEYS_MIXED, None)
            O.inner_device(engine, table, d_pk, d_st, _up(engine, epoch).view(torch.int64), d_arena, d_plain, d_fw, d_in)
            if ct is not None:
                ct.lookup_device(d_fw, d_in, n, now, d_v, d_c, d_plain=d_plain, d_work=d_work, work_cap=n)
            O.coalesce_batch_device(engine, d_plain, d_arena, d_out[:cap], d_writes, d_nw, d_pw, d_ps)
            torch.cuda.synchronize(dev)
            dw.destroy()
            dw = None
            nw = int(d_nw.item())
            return dict(writes=d_writes.cpu().numpy().view(L.TUN_WRITE_DTYPE)[:nw].copy(), out=d_out.cpu().numpy(),
                        pw=d_pw.cpu().numpy().view(np.uint32), inner=d_in.cpu().numpy(), fw=d_fw.cpu().numpy().view(L.FW_PACKET_DTYPE),
                        verdict=d_v.cpu().numpy(), counts=d_c.cpu().numpy().tolist(),
                        work=d_work.cpu().numpy().view(L.CT_WORK_DTYPE), plain=d_plain.cpu().numpy().view(L.PLAIN_PACKET_DTYPE))

        with PeerTable(engine, 16) as table, F.Conntrack(engine, 64, seed=9, max_batch=512) as ct:
            table.set_routable(routable(RC.MY_NETWORKS, RC.MY_UNSAFE))
            table.update(put=[(ciphers[t].key_id, f"10.1.0.{20 + t}/32", L.NET_VPN) for t in range(ntun)])
            base = receive(None, 0)
            good = base["inner"] == L.STATUS_OK
            assert good.sum() > 150 and (base["pw"][good] != L.WRITE_NONE).all()
            # nothing tracked: every packet the inner resolve passed is held, and the TUN gets nothing
            held = receive(ct, K.T0)
            assert (held["pw"] == L.WRITE_NONE).all() and len(held["writes"]) == 0
            assert (held["verdict"] == np.where(good, L.CT_MISS, L.CT_NONE)).all()
            assert (held["inner"] == np.where(good, L.STATUS_FW_HELD, base["inner"])).all()
            ng = int(good.sum())
            assert held["counts"] == [0, ng, 0, ng] and held["work"]["packet"][:ng].tolist() == np.flatnonzero(good).tolist()
            assert held["work"]["fw"][:ng].tobytes() == base["fw"][good].tobytes()
            # the caller's rules admit tunnels 0 and 2: their flows from the work list, once each
            flows = {}
            for w in held["work"][:ng]:
                if tunnel_of[w["packet"]] != 1:
                    flows.setdefault(R.keys_of(w["fw"].reshape(1))[0], w["fw"])
            admitted = np.array(list(flows.values()), L.FW_PACKET_DTYPE)
            res = DeviceRunner(engine, ct).add(admitted, [1] * len(admitted), K.T0)
            assert (res["code"] == L.CT_NEW).all() and len(admitted) == 2
            some = receive(ct, K.T0 + 1)
            hit = good & (tunnel_of != 1)
            assert (some["verdict"] == np.where(hit, L.CT_HIT, np.where(good, L.CT_MISS, L.CT_NONE))).all()
            assert ((some["pw"] != L.WRITE_NONE) == hit).all()  # held packets are absent from the TUN output, hits present
            for w in some["writes"]:
                assert tunnel_of[w["first"]] != 1
            assert (some["plain"]["flags"][good & ~hit] & L.PLAIN_SKIP).all() and not (some["plain"]["flags"][hit] & L.PLAIN_SKIP).any()
            # every flow tracked: byte-identical to the run without the call
            rest = np.array([w["fw"] for w in some["work"][:some["counts"][3]]][:1], L.FW_PACKET_DTYPE)
            assert (DeviceRunner(engine, ct).add(rest, [1], K.T0 + 1)["code"] == L.CT_NEW).all()
            full = receive(ct, K.T0 + 2)
            assert full["counts"] == [ng, 0, 0, 0]
            used = int(base["writes"][-1]["out_off"]) + int(base["writes"][-1]["len"])
            assert full["writes"].tobytes() == base["writes"].tobytes() and full["out"][:used].tobytes() == base["out"][:used].tobytes()
            assert (full["pw"] == base["pw"]).all() and (full["inner"] == base["inner"]).all()
            assert full["plain"].tobytes() == base["plain"].tobytes()
    finally:
        if dw is not None:
            dw.destroy()
        for c in ciphers:
            c.destroy()


# ---- and on the TX side: resolve -> lookup -> seal -----------------------------------------------------

def test_behind_the_tx_resolve_in_front_of_the_seal(engine):
    import torch

    import tx_resolve_cases as TC
    from nebula_amd.hostmap import TxTable
    from nebula_amd.inside import TX_TUNNEL_DTYPE, DeviceTxBatch
    from nebula_amd.noiseutil import CipherAESGCM
    from test_gpu_tx_resolve import _tx_batch

    case = TC.build()
    rng = random.Random(41)
    pk, arena, model = _tx_batch(case)
    n, ntun = len(pk), 20
    ciphers = [CipherAESGCM.Cipher(engine, bytes(rng.getrandbits(8) for _ in range(32))) for _ in range(ntun)]
    try:
        tun = np.zeros(ntun, TX_TUNNEL_DTYPE)
        for k, c in enumerate(ciphers):
            tun[k] = (100 * k + 1, c.key_id, 0xB000 + k)
        pk["tunnel"] = 0xEEEEEEEE

        def send(table, ct, now):
            db = DeviceTxBatch(engine, L.ALG_AESGCM, tun, pk, arena, 1 << 18, 512)
            d_fw, d_st = _fill(engine, n * FW, 0xEE, torch.uint8), _fill(engine, n, -7, torch.int32)
            d_v, d_c = _fill(engine, n, 0xEE, torch.uint8), _fill(engine, 4, -7, torch.int32)
            torch.cuda.synchronize()
            table.resolve_device(db.packets, db.inp, d_fw, d_st)
            if ct is not None:
                ct.lookup_device(d_fw, d_st, n, now, d_v, d_c, d_tx=db.packets)
            db.seal()  # on the same stream
            torch.cuda.synchronize()
            r = db.result()
            return dict(r=r, st=d_st.cpu().numpy(), fw=d_fw.cpu().numpy().view(L.FW_PACKET_DTYPE), v=d_v.cpu().numpy(),
                        counts=d_c.cpu().numpy().tolist(), tunnel=db.packets.cpu().numpy().view(TX_PACKET_DTYPE)["tunnel"])

        def same(a, b):
            return all(x.tobytes() == y.tobytes() for x, y in ((a.wires, b.wires), (a.wire_status, b.wire_status),
                                                               (a.packet_status, b.packet_status), (a.out, b.out), (a.tunnels, b.tunnels)))

        with TxTable(engine, TC.HOSTS, TC.ROUTES, TC.GATEWAYS) as t, \
                F.Conntrack(engine, 256, seed=11, max_batch=256) as ct:
            TC.load(t, case)
            base = send(t, None, 0)
            ok = base["st"] == L.STATUS_OK
            sealed = base["r"].packet_status == L.STATUS_OK
            assert ok.sum() >= 20 and sealed.sum() >= 20 and not (sealed & ~ok).any()
            # nothing tracked: every resolved read is held, nothing is sealed, no counter moves
            none = send(t, ct, K.T0)
            assert (none["v"] == np.where(ok, L.CT_MISS, L.CT_NONE)).all() and (none["tunnel"] == L.TX_NO_TUNNEL).all()
            assert (none["st"] == np.where(ok, L.STATUS_FW_HELD, base["st"])).all()
            assert len(none["r"].wires) == 0 and not (none["r"].packet_status == L.STATUS_OK).any()
            assert none["r"].tunnels.tobytes() == tun.tobytes()
            # the flows of every other resolved read are admitted (copies of one flow come along)
            idx = np.flatnonzero(ok)[::2]
            DeviceRunner(engine, ct).add(base["fw"][idx], [0] * len(idx), K.T0)
            tracked = set(R.keys_of(base["fw"][idx]))
            hit = np.array([o and k in tracked for o, k in zip(ok, R.keys_of(base["fw"]))])
            half = send(t, ct, K.T0 + 1)
            assert (half["v"] == np.where(hit, L.CT_HIT, np.where(ok, L.CT_MISS, L.CT_NONE))).all() and (ok & ~hit).any()
            pst = half["r"].packet_status
            assert (pst[hit] == base["r"].packet_status[hit]).all()
            assert np.isin(pst[ok & ~hit], (L.STATUS_BAD_KEY, L.STATUS_INVALID)).all()  # held reads are not sealed
            assert (half["tunnel"][hit] == base["tunnel"][hit]).all() and (half["tunnel"][~hit] == L.TX_NO_TUNNEL).all()
            assert 0 < len(half["r"].wires) < len(base["r"].wires)
            # all tracked: the seal gives what it gives without the call
            rest = np.flatnonzero(ok & ~hit)
            DeviceRunner(engine, ct).add(base["fw"][rest], [0] * len(rest), K.T0 + 1)
            full = send(t, ct, K.T0 + 2)
            assert full["counts"] == [int(ok.sum()), 0, 0, 0] and same(full["r"], base["r"])
            assert (full["st"] == base["st"]).all() and (full["tunnel"] == base["tunnel"]).all()
    finally:
        for c in ciphers:
            c.destroy()
