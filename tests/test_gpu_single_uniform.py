"""The single-key kernel's uniform-round loop (gcm_packet_group: waves whose 16 packets share one
(aad_len, len) run their full-block rounds with a scalar trip count and running pointers) through
the C ABI against the oracle, bit-exact.

One key with key_hint set and 6160 packets per batch: just over kSmallBatch = 6144, so
gcm_single_kernel runs and not the tail kernel. Uniform batches at the lengths where the peeled
rounds differ (pad 0-3, a partial last block, one and two rounds: no interior round at all), a
1300-B batch with a few odd packets (their waves take the general loop beside uniform neighbours),
invalid lanes in the last group, an arena off 16-byte and off 4-byte alignment (general loop), a
flipped tag in a uniform wave, and out-of-place seal and open. The oracle alone decides each case."""
import numpy as np
import pytest

from nebula_amd import _lib as L
from nebula_amd import workload as W

from test_gpu_parity import oracle_open, oracle_seal, run_device

pytestmark = pytest.mark.gpu

N = 6160
# 1300: n = 84 blocks, no pad, 4-byte last block; 1296 / 1280 / 1264: pad 1 / 2 / 3; 1281: one byte
# in the last block; 52 and 16: two rounds and one round (no interior round)
UNIFORM_LENS = (1300, 1296, 1280, 1264, 1281, 52, 16)
_CACHE = {}


def _sealed_opened(oracle_mod, b):
    ref, st = oracle_seal(oracle_mod, b)
    assert (st == 0).all()
    ref_o, st_o = oracle_open(oracle_mod, b, ref)
    assert (st_o == 0).all()
    return b, ref, ref_o


def _uniform(oracle_mod, ln, n=N):
    """A batch of n packets of ln bytes, its oracle-sealed arena and the oracle's opening of it."""
    key = ("uniform", ln, n)
    if key not in _CACHE:
        b = W.make_batch(L.ALG_AESGCM, n, 1, sizes=(ln,), seed=0x0A11 + ln, name=f"uniform-{ln}")
        assert b.n == n > 6144 and b.nkeys == 1 and (b.desc["aad_len"] == 16).all()
        _CACHE[key] = _sealed_opened(oracle_mod, b)
    return _CACHE[key]


# nearly uniform: packet -> length, each in a wave (16 consecutive packets) of its own
ODD = {5 * 16 + 3: 1299, 100 * 16: 1284, 200 * 16 + 15: 0, 384 * 16 + 9: 1299}
EXHAUSTED, FOREIGN = 50 * 16 + 7, 60 * 16 + 2


def _nearly(oracle_mod):
    if "nearly" not in _CACHE:
        base = _uniform(oracle_mod, 1300)[0]
        d = base.desc.copy()
        for p, ln in ODD.items():
            d["len"][p] = ln
        b = W.Batch(base.alg, base.keys, base.remote_index, d, base.arena, base.stride, "nearly-uniform")
        _CACHE["nearly"] = _sealed_opened(oracle_mod, b)
    return _CACHE["nearly"]


def _out_of_place(oracle_mod):
    """1300-B packets sealed from the first half of a slot into its second half, and the batch that
    opens them back the other way (over plaintext bytes overwritten first)."""
    if "oop" not in _CACHE:
        base = _uniform(oracle_mod, 1300)[0]
        stride = 2 * base.stride
        arena = np.zeros(N * stride, np.uint8)
        arena.reshape(N, stride)[:, :base.stride] = base.arena.reshape(N, base.stride)
        d = base.desc.copy()
        slot = np.arange(N, dtype=np.uint64) * np.uint64(stride)
        d["aad_off"], d["src_off"] = slot, slot + np.uint64(16)
        d["dst_off"] = slot + np.uint64(base.stride + 16)
        assert (d["dst_off"] % 16 == 0).all()
        b = W.Batch(base.alg, base.keys, base.remote_index, d, arena, stride, "uniform-oop")
        ref, st = oracle_seal(oracle_mod, b)
        assert (st == 0).all()
        do = d.copy()
        do["src_off"], do["dst_off"] = d["dst_off"], d["src_off"]
        ob = W.Batch(base.alg, base.keys, base.remote_index, do, arena, stride, "uniform-oop-open")
        t = ref.copy()
        t.reshape(N, stride)[:, 16:16 + 1300] ^= 0xA5  # the open has to write every plaintext byte
        ref_o, st_o = oracle_open(oracle_mod, ob, t)
        assert (st_o == 0).all()
        assert np.array_equal(ref_o.reshape(N, stride)[:, :16 + 1300], arena.reshape(N, stride)[:, :16 + 1300])
        _CACHE["oop"] = (b, ref, ob, t, ref_o)
    return _CACHE["oop"]


@pytest.mark.parametrize("ln", UNIFORM_LENS)
def test_uniform_seal_matches_oracle(engine, oracle_mod, ln):
    b, ref, _ = _uniform(oracle_mod, ln)
    got, st = run_device(engine, b, seal=True)
    assert (st == 0).all()
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("ln", UNIFORM_LENS)
def test_uniform_open_restores_plaintext(engine, oracle_mod, ln):
    b, ref, ref_o = _uniform(oracle_mod, ln)
    got, st = run_device(engine, b, seal=False, arena=ref)
    assert (st == 0).all()
    assert np.array_equal(got, ref_o)
    assert np.array_equal(got.reshape(N, b.stride)[:, :16 + ln], b.arena.reshape(N, b.stride)[:, :16 + ln])


@pytest.mark.parametrize("ln", UNIFORM_LENS)
def test_uniform_flipped_tag_fails_that_packet_alone(engine, oracle_mod, ln):
    """A flipped byte of the received tag in a uniform wave fails that packet, zeroes its payload
    and leaves its header, its tag and every other packet as the oracle has them."""
    b, ref, ref_o = _uniform(oracle_mod, ln)
    victim = 3001
    s = int(b.desc["src_off"][victim])
    bad = ref.copy()
    bad[s + ln + 9] ^= 0x20
    exp, st_exp = oracle_open(oracle_mod, b, bad)
    assert st_exp[victim] == L.STATUS_AUTH_FAILED and not exp[s:s + ln].any()
    got, st = run_device(engine, b, seal=False, arena=bad)
    assert st[victim] == L.STATUS_AUTH_FAILED
    assert (np.delete(st, victim) == 0).all()
    assert np.array_equal(got, exp)
    others = np.delete(np.arange(N), victim)
    assert np.array_equal(got.reshape(N, b.stride)[others], ref_o.reshape(N, b.stride)[others])


def test_nearly_uniform_waves(engine, oracle_mod):
    """1300 B everywhere but one packet of 1299, 1284 or 0 bytes in a few waves: those waves run the
    general loop, their neighbours the uniform one."""
    b, ref, ref_o = _nearly(oracle_mod)
    got, st = run_device(engine, b, seal=True)
    assert (st == 0).all()
    assert np.array_equal(got, ref)
    got_o, st_o = run_device(engine, b, seal=False, arena=ref)
    assert (st_o == 0).all()
    assert np.array_equal(got_o, ref_o)


def test_nearly_uniform_exhausted_and_foreign_key(engine, oracle_mod):
    """A counter at NEB_REJECT_AFTER_MESSAGES and a foreign key_id, each in an otherwise uniform
    wave: EXHAUSTED and BAD_KEY for those two, nothing of theirs written, every other packet sealed."""
    b, ref, _ = _nearly(oracle_mod)
    d = b.desc.copy()
    d["counter"][EXHAUSTED] = L.REJECT_AFTER_MESSAGES
    d["key_id"][FOREIGN] = 7000  # not this batch's key
    got, st = run_device(engine, b, seal=True, desc=d)
    assert st[EXHAUSTED] == L.STATUS_EXHAUSTED and st[FOREIGN] == L.STATUS_BAD_KEY
    assert (np.delete(st, [EXHAUSTED, FOREIGN]) == 0).all()
    exp = ref.reshape(N, b.stride).copy()
    exp[[EXHAUSTED, FOREIGN]] = b.arena.reshape(N, b.stride)[[EXHAUSTED, FOREIGN]]
    assert np.array_equal(got.reshape(N, b.stride), exp)


def test_invalid_lanes_in_last_group(engine, oracle_mod):
    n = 6165  # the last group holds 5 packets
    b, ref, ref_o = _uniform(oracle_mod, 1300, n)
    got, st = run_device(engine, b, seal=True)
    assert (st == 0).all()
    assert np.array_equal(got, ref)
    got_o, st_o = run_device(engine, b, seal=False, arena=ref)
    assert (st_o == 0).all()
    assert np.array_equal(got_o, ref_o)


@pytest.mark.parametrize("shift", [4, 1])
def test_misaligned_arena_takes_general_loop(engine, oracle_mod, shift):
    """The arena at a +4-byte and a +1-byte view of its buffer: no destination is 16-byte aligned
    (and at +1 no source 4-byte aligned), so every wave runs the general loop."""
    import torch

    from nebula_amd.batch import DeviceBatch, install_keys

    b, ref, ref_o = _uniform(oracle_mod, 1300)
    ciphers = install_keys(engine, b)
    try:
        db = DeviceBatch(engine, b, ciphers)
        big = torch.zeros(b.arena.nbytes + 16, dtype=torch.uint8, device=db.dev)
        db.arena = big[shift:shift + b.arena.nbytes]
        db.arena.copy_(torch.from_numpy(b.arena))
        assert db.arena.data_ptr() % 16 == shift
        db.seal()
        torch.cuda.synchronize()
        assert (db.status_host() == 0).all()
        assert np.array_equal(db.arena_host(), ref)
        db.open()
        torch.cuda.synchronize()
        assert (db.status_host() == 0).all()
        assert np.array_equal(db.arena_host(), ref_o)
        assert not big[:shift].any() and not big[shift + b.arena.nbytes:].any()  # nothing outside
    finally:
        for c in ciphers:
            c.destroy()


def test_out_of_place_seal_and_open(engine, oracle_mod):
    b, ref, ob, t, ref_o = _out_of_place(oracle_mod)
    got, st = run_device(engine, b, seal=True)
    assert (st == 0).all()
    assert np.array_equal(got, ref)
    got_o, st_o = run_device(engine, ob, seal=False, arena=t)
    assert (st_o == 0).all()
    assert np.array_equal(got_o, ref_o)
