"""GPU: the per-packet CipherState surface, mirroring noiseutil/cipher_state_test.go and
noiseutil/fips140_test.go case by case (through nebula_amd.noiseutil -> C ABI -> gfx950 kernels)."""
import json
import os

import numpy as np
import pytest

from nebula_amd import _lib as L
from nebula_amd import noiseutil as N
from nebula_amd.noiseutil import Slice

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEY = bytes(range(32))


def build_cipher_states(engine, cf):
    """Stand-in for buildCipherStates (cipher_state_test.go:51-76): both sides share one key."""
    enc = N.NewCipherState((engine, KEY), cf)
    dec = N.NewCipherState((engine, KEY), cf)
    return enc, dec


@pytest.mark.parametrize("cf", [N.CipherAESGCM, N.CipherChaChaPoly], ids=["AESGCM", "ChaChaPoly"])
def test_roundtrip(engine, cf):  # cipher_state_test.go:13-21,78-98
    enc, dec = build_cipher_states(engine, cf)
    plaintext = b"nebula cipher state roundtrip"
    ad = b"aad"
    nb = bytearray(12)
    ct = enc.EncryptDanger(None, ad, plaintext, 1, nb)
    assert ct.bytes() != plaintext
    pt = dec.DecryptDanger(None, ad, ct, 1, nb)
    assert pt.bytes() == plaintext
    with pytest.raises(N.ErrOpen):
        dec.DecryptDanger(None, ad, ct, 2, nb)
    assert enc.Overhead() == dec.Overhead() == 16
    enc.destroy(), dec.destroy()


def test_dispatch_and_unsupported(engine):  # cipher_state_test.go:23-49
    a, _ = build_cipher_states(engine, N.CipherAESGCM)
    c, _ = build_cipher_states(engine, N.CipherChaChaPoly)
    assert isinstance(a, N.CipherStateAESGCM) and isinstance(c, N.CipherStateChaChaPoly)
    assert N.NewCipherState(a, N.CipherAESGCM) is a  # plugin hook cipher_state.go:43-45
    with pytest.raises(RuntimeError):
        N.NewCipherState((engine, KEY), N.CipherFunc("Fake", 99))
    assert N.CipherAESGCM.CipherName() == "AESGCM" and N.CipherChaChaPoly.CipherName() == "ChaChaPoly"
    for cs in list(engine.live.values()):
        cs.destroy()


@pytest.mark.parametrize("cf", [N.CipherAESGCM, N.CipherChaChaPoly], ids=["AESGCM", "ChaChaPoly"])
def test_encrypt_rejects_exhausted_counter(engine, cf):  # cipher_state_test.go:100-116
    assert N.RejectHeadroom == 1 << 40
    assert N.RejectAfterMessages == (1 << 64) - 1 - N.RejectHeadroom
    enc, _ = build_cipher_states(engine, cf)
    nb = bytearray(12)
    enc.EncryptDanger(None, None, b"x", N.RejectAfterMessages - 1, nb)
    with pytest.raises(N.ErrMessageCounterExhausted):
        enc.EncryptDanger(None, None, b"x", N.RejectAfterMessages, nb)
    for cs in list(engine.live.values()):
        cs.destroy()


def test_nil_safety():  # cipher_state_test.go:176-192
    for cls in (N.CipherStateAESGCM, N.CipherStateChaChaPoly):
        nil = cls.nil()
        with pytest.raises(N.ErrNoCipher):
            nil.EncryptDanger(None, None, None, 0, bytearray(12))
        out = nil.DecryptDanger(None, None, None, 0, bytearray(12))
        assert len(out) == 0
        assert nil.Overhead() == 0


@pytest.mark.parametrize("cf", [N.CipherAESGCM, N.CipherChaChaPoly], ids=["AESGCM", "ChaChaPoly"])
def test_in_place_decrypt(engine, cf):  # cipher_state_test.go:194-237
    enc, dec = build_cipher_states(engine, cf)
    hdr_len = 16
    plaintext = b"in-place decrypt should replace the ciphertext bytes"
    nb = bytearray(12)
    packet = Slice.make(hdr_len, hdr_len + len(plaintext) + enc.Overhead())
    for i in range(hdr_len):
        packet.buf[i] = i
    packet = enc.EncryptDanger(packet, packet[:hdr_len], plaintext, 1, nb)
    assert len(packet) == hdr_len + len(plaintext) + 16
    assert packet.bytes()[:hdr_len] == bytes(range(16))  # ad aliased out: header kept

    neighbor = b"next coalesced segment, must stay intact"
    row = Slice(bytearray(packet.bytes() + neighbor))
    tampered = row[:len(packet)]
    tampered.buf[hdr_len] ^= 0x01
    with pytest.raises(N.ErrOpen):
        dec.DecryptDanger(tampered[hdr_len:hdr_len], tampered[:hdr_len], tampered[hdr_len:], 1, nb)
    assert tampered.bytes()[:hdr_len] == packet.bytes()[:hdr_len]
    assert tampered.bytes()[-16:] == packet.bytes()[-16:]
    assert row.bytes()[len(packet):] == neighbor

    out = dec.DecryptDanger(packet[hdr_len:hdr_len], packet[:hdr_len], packet[hdr_len:], 1, nb)
    assert out.bytes() == plaintext
    assert out.same_element(packet[hdr_len:])  # plaintext aliases the packet buffer
    enc.destroy()
    dec.destroy()


def test_reference_aesgcm_kat_through_encrypt_danger(engine):  # fips140_test.go:13-31
    k = json.load(open(os.path.join(GOLD, "kat.json")))["aesgcm_fips140_test"]
    cs = N.CipherAESGCM.Cipher(engine, bytes.fromhex(k["key"]))
    nb = bytearray(12)
    out = cs.EncryptDanger(None, bytes.fromhex(k["aad"]), bytes.fromhex(k["plaintext"]),
                           int(k["nebula_counter"], 16), nb)
    assert bytes(nb).hex() == k["iv"]
    assert out.bytes().hex() == k["expected"]
    cs.destroy()


def test_rfc8439_through_engine(engine):
    """ChaCha nonce is 00000000 || LE64(n); RFC 8439's nonce 07000000 4041424344454647 has a
    non-zero first word, so compare with the oracle on Nebula's own nonce instead, and check the
    RFC vector through the oracle-pinned tag (tests/test_oracle.py)."""
    import oracle

    k = json.load(open(os.path.join(GOLD, "kat.json")))["chachapoly_rfc8439_2_8_2"]
    key, aad, pt = bytes.fromhex(k["key"]), bytes.fromhex(k["aad"]), bytes.fromhex(k["plaintext"])
    n = 0x4746454443424140
    cs = N.CipherChaChaPoly.Cipher(engine, key)
    out = cs.EncryptDanger(None, aad, pt, n)
    assert out.bytes() == oracle.seal(2, key, oracle.nonce(2, n), aad, pt)
    cs.destroy()


@pytest.mark.parametrize("cf", [N.CipherAESGCM, N.CipherChaChaPoly], ids=["AESGCM", "ChaChaPoly"])
def test_append_semantics(engine, cf):
    """EncryptDanger appends after out[:len]; a too-small cap grows into a new array like Go."""
    cs = cf.Cipher(engine, KEY)
    out = Slice.make(3, 3)
    out.buf[:3] = b"abc"
    r = cs.EncryptDanger(out, b"", b"hello", 9)
    assert r.bytes()[:3] == b"abc" and len(r) == 3 + 5 + 16
    assert r.buf is not out.buf
    big = Slice.make(3, 64)
    big.buf[:3] = b"abc"
    r2 = cs.EncryptDanger(big, b"", b"hello", 9)
    assert r2.buf is big.buf and r2.bytes() == r.bytes()
    with pytest.raises(N.ErrOpen):  # ciphertext shorter than the tag
        cs.DecryptDanger(None, b"", b"0123456789", 9)
    cs.destroy()


def test_concurrent_encrypt_decrypt_danger(engine, oracle_mod):
    """EncryptDanger / DecryptDanger from 16 threads at once on shared CipherStates (Nebula calls
    them from every routine, lock-free: noiseutil/notboring.go:12): 16 threads over the engine's
    fixed pool of 4 slots, and every output equals the oracle's."""
    import threading

    from nebula_amd import _lib as L
    from nebula_amd.noiseutil import CipherAESGCM, CipherChaChaPoly

    rng = np.random.default_rng(11)
    states = []
    for i in range(4):
        cf = CipherAESGCM if i % 2 == 0 else CipherChaChaPoly
        k = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        states.append((cf.Cipher(engine, k), k, L.ALG_AESGCM if i % 2 == 0 else L.ALG_CHACHAPOLY))
    errors = []

    def worker(t):
        try:
            r = np.random.default_rng(100 + t)
            for j in range(150):
                cs, k, alg = states[(t + j) % 4]
                n = (t << 32) | j
                pt = bytes(r.integers(0, 256, int(r.choice([0, 1, 100, 1300])), dtype=np.uint8))
                ad = bytes(r.integers(0, 256, 16, dtype=np.uint8))
                ct = cs.EncryptDanger(None, ad, pt, n).bytes()
                ref = oracle_mod.seal(alg, k, oracle_mod.nonce(alg, n), ad, pt)
                if ct != ref:
                    raise AssertionError(f"seal mismatch t={t} j={j}")
                if cs.DecryptDanger(None, ad, ct, n).bytes() != pt:
                    raise AssertionError(f"open mismatch t={t} j={j}")
        except Exception as ex:
            errors.append(ex)

    ths = [threading.Thread(target=worker, args=(t,)) for t in range(16)]
    try:
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errors, errors[:3]
    finally:
        for cs, _, _ in states:
            cs.destroy()


def test_destroy_does_not_wait_for_another_tunnels_batch(engine, oracle_mod):
    """neb_cipher_destroy waits only for batches that may read the destroyed key. Another tunnel's
    single-key batches are queued on a stream behind a host gate (hipLaunchHostFunc blocking on a
    threading.Event), so they cannot run until the test opens it: the destroy of an unrelated key
    must return while they are still queued (the old device-wide drain would block until the gate
    opened). Ordering only, no wall-clock bound: the batch's end event is still pending when the
    destroy returns, and the batches then complete correctly."""
    import ctypes as C
    import threading

    import torch

    from nebula_amd import workload as W
    from nebula_amd.batch import DeviceBatch, install_keys
    from nebula_amd.noiseutil import CipherAESGCM

    hip = None
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            hip = C.CDLL(line.split()[-1])
            break
    assert hip is not None
    gate = threading.Event()
    HOSTFN = C.CFUNCTYPE(None, C.c_void_p)
    hostfn = HOSTFN(lambda _: gate.wait(60))  # (a bound: a broken destroy cannot hang the suite)

    b = W.make_batch(1, 65536, 1, name="long")
    ciphers = install_keys(engine, b)
    other = CipherAESGCM.Cipher(engine, bytes(range(32)))
    try:
        db = DeviceBatch(engine, b, ciphers)
        s = torch.cuda.Stream()
        db.seal(stream=s.cuda_stream)  # warm
        s.synchronize()
        ev_end = torch.cuda.Event()
        try:
            assert hip.hipLaunchHostFunc(C.c_void_p(s.cuda_stream), hostfn, None) == 0
            for _ in range(4):
                db.seal(stream=s.cuda_stream)
            ev_end.record(s)
            done = threading.Event()
            th = threading.Thread(target=lambda: (other.destroy(), done.set()))
            th.start()
            returned = done.wait(20)
            pending = not ev_end.query()
        finally:
            gate.set()
        th.join(60)
        s.synchronize()
        assert returned, "the destroy waited for another tunnel's queued batch"
        assert pending, "the gated batch ran before the gate opened"
        assert (db.status_host() == 0).all()
    finally:
        gate.set()
        for c in ciphers:
            c.destroy()


def test_per_packet_pool_bounded_over_many_engines(oracle_mod):
    """One thread alternating over 10 engines (round 3's 8-entry per-thread cache leaked a stream and
    a pinned buffer per call here): every engine keeps its fixed pool of 4 slots, and every packet
    still equals the oracle. Then 48 threads on one engine: still 4 slots, FIFO turns."""
    import threading

    from nebula_amd import _lib as L
    from nebula_amd.noiseutil import CipherAESGCM, Engine

    engines = [Engine(0, max_keys=4) for _ in range(10)]
    try:
        keys = [bytes([i + 1] * 32) for i in range(10)]
        cs = [CipherAESGCM.Cipher(e, k) for e, k in zip(engines, keys)]
        for j in range(5):
            for i, (c, k) in enumerate(zip(cs, keys)):
                n = j * 10 + i
                pt = bytes([j, i]) * 300
                ct = c.EncryptDanger(None, b"h" * 16, pt, n).bytes()
                assert ct == oracle_mod.seal(L.ALG_AESGCM, k, oracle_mod.nonce(L.ALG_AESGCM, n), b"h" * 16, pt)
        for e in engines:
            st = e.stats()
            assert st["pkt_slots"] == 4 and st["pkt_calls"] >= 5
        errors = []

        def worker(t):
            try:
                for j in range(20):
                    pt = bytes([t, j]) * 50
                    ct = cs[0].EncryptDanger(None, b"", pt, t * 100 + j)
                    if cs[0].DecryptDanger(None, b"", ct, t * 100 + j).bytes() != pt:
                        raise AssertionError(f"round trip t={t} j={j}")
            except Exception as ex:
                errors.append(ex)

        ths = [threading.Thread(target=worker, args=(t,)) for t in range(48)]
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errors, errors[:3]
        st = engines[0].stats()
        assert st["pkt_slots"] == 4 and st["pkt_calls"] >= 48 * 40
        for c in cs:
            c.destroy()
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("alg", [1, 2])
def test_cipher_create_batch_c3_shape(oracle_mod, alg):
    """4096 tunnel keys installed by one neb_cipher_create_batch (one launch), then a C3-shaped batch
    (16 packets per key on average) sealed and opened through them, bit-exact against the oracle."""
    import torch

    from nebula_amd import workload as W
    from nebula_amd.batch import DeviceBatch, install_keys
    from nebula_amd.noiseutil import Engine

    b = W.make_batch(alg, 8192, 4096, seed=41, name="batch-install")
    ref = b.arena.copy()
    assert (oracle_mod.batch(alg, 0, b.keys, b.desc, ref) == 0).all()
    with Engine(0, 4096) as eng:
        cs = install_keys(eng, b)
        assert len(cs) == 4096 and sorted(c.key_id for c in cs) == list(range(4096))
        assert eng.stats()["installs"] == 4096
        db = DeviceBatch(eng, b, cs)
        db.seal()
        torch.cuda.synchronize()
        assert (db.status_host() == 0).all()
        assert np.array_equal(db.arena_host(), ref)
        db.open()
        torch.cuda.synchronize()
        exp = ref.copy()
        oracle_mod.batch(alg, 1, b.keys, b.desc, exp)
        assert (db.status_host() == 0).all() and np.array_equal(db.arena_host(), exp)
        for c in cs[::2]:
            c.destroy()
        # reinstall over freed slots, another algorithm's records cleared on the way
        other = 3 - alg
        b2 = W.make_batch(other, 512, 2048, seed=42, name="reinstall")
        cs2 = install_keys(eng, b2)
        assert sorted(c.key_id for c in cs2) == list(range(0, 4096, 2))
        ref2 = b2.arena.copy()
        assert (oracle_mod.batch(other, 0, b2.keys, b2.desc, ref2) == 0).all()
        db2 = DeviceBatch(eng, b2, cs2)
        db2.seal()
        torch.cuda.synchronize()
        assert (db2.status_host() == 0).all() and np.array_equal(db2.arena_host(), ref2)
        for c in cs[1::2] + cs2:
            c.destroy()


def test_entry_points_restore_current_device():
    """Every entry point restores the caller's current HIP device (hip_guard.hpp). With two or more
    devices an engine on device 1 is driven while torch's current device is 0."""
    import torch

    from nebula_amd import _lib as L
    from nebula_amd import workload as W
    from nebula_amd.batch import DeviceBatch, host_batch, install_keys, slot_desc
    from nebula_amd.noiseutil import CipherAESGCM, Engine

    ndev = torch.cuda.device_count()
    dev = 1 if ndev > 1 else 0
    torch.cuda.set_device(0)
    b = W.make_batch(L.ALG_AESGCM, 300, 3, seed=7, name="guard")
    with Engine(dev, 16) as eng:
        assert torch.cuda.current_device() == 0
        cs = install_keys(eng, b)
        c1 = CipherAESGCM.Cipher(eng, bytes(32))
        assert torch.cuda.current_device() == 0
        c1.EncryptDanger(None, b"", b"x" * 40, 1)
        assert torch.cuda.current_device() == 0
        host_batch(eng, L.ALG_AESGCM, False, slot_desc(b, cs), b.arena.copy())
        assert torch.cuda.current_device() == 0
        db = DeviceBatch(eng, b, cs, device=dev)
        db.seal(stream=torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        assert torch.cuda.current_device() == 0
        for c in cs + [c1]:
            c.destroy()
        assert torch.cuda.current_device() == 0
    assert torch.cuda.current_device() == 0


def test_one_packet_kernel_size_boundary(engine, oracle_mod):
    """AES-GCM per-packet calls carry the packet in the kernel's arguments up to 2048 bytes of
    AAD (padded to 16) + payload (+ tag when opening) (aes_gcm.hip gcm_one_kernel); larger ones take
    the batch path. Both sides of the boundary, with 0-, 16- and 1348-byte AADs (the relay's
    GMAC), seal and open against the oracle, a tampered tag refused with the plaintext zeroed."""
    from nebula_amd import _lib as L
    from nebula_amd.noiseutil import CipherAESGCM

    rng = np.random.default_rng(5)
    key = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    cs = CipherAESGCM.Cipher(engine, key)
    try:
        for ad_len in (0, 16, 1348):
            room = 2048 - ((ad_len + 15) // 16) * 16
            for pt_len in sorted({0, 1, 15, 16, 17, room - 17, room - 16, room - 15, room - 1, room, room + 1, 4000}):
                n = (ad_len << 20) | pt_len
                ad = bytes(rng.integers(0, 256, ad_len, dtype=np.uint8))
                pt = bytes(rng.integers(0, 256, pt_len, dtype=np.uint8))
                ct = cs.EncryptDanger(None, ad, pt, n).bytes()
                assert ct == oracle_mod.seal(L.ALG_AESGCM, key, oracle_mod.nonce(L.ALG_AESGCM, n), ad, pt), (ad_len, pt_len)
                assert cs.DecryptDanger(None, ad, ct, n).bytes() == pt, (ad_len, pt_len)
                bad = bytearray(ct)
                bad[-1] ^= 1
                with pytest.raises(N.ErrOpen):
                    cs.DecryptDanger(None, ad, bytes(bad), n)
    finally:
        cs.destroy()


def test_concurrent_calls_combined_with_forgeries(engine, oracle_mod):
    """Concurrent AES-256-GCM calls that the engine combines into one launch (engine.cpp PktComb:
    calls arriving while another launch is made ride together): 24 threads over 6 tunnels, payloads
    0-1400 B with AAD up to 48 B (whole blocks and not), every 5th open given a flipped ciphertext or
    tag bit — that call alone must fail (ErrOpen, its output zeroed) while the others in the same
    launch succeed, every byte against the oracle. How many calls combine here is a matter of
    timing, so nothing below asserts it: the combined kernel is pinned slot by slot by
    tests/test_gpu_pkt_combined.py (deterministic launches through neb_engine_pkt_launch) and the
    leader/joiner protocol by tests/sanitize/comb_test.cpp (launches held and released on a fake
    device)."""
    import threading

    from nebula_amd.noiseutil import CipherAESGCM, ErrOpen

    rng = np.random.default_rng(23)
    states = []
    for _ in range(6):
        k = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
        states.append((CipherAESGCM.Cipher(engine, k), k))
    errors = []

    def worker(t):
        try:
            r = np.random.default_rng(500 + t)
            for j in range(120):
                cs, k = states[(t * 5 + j) % 6]
                n = (t << 40) | j
                pt = bytes(r.integers(0, 256, int(r.choice([0, 1, 15, 16, 17, 90, 576, 1300, 1400])), dtype=np.uint8))
                ad = bytes(r.integers(0, 256, int(r.choice([0, 1, 13, 16, 17, 48])), dtype=np.uint8))
                ct = cs.EncryptDanger(None, ad, pt, n).bytes()
                if ct != oracle_mod.seal(L.ALG_AESGCM, k, oracle_mod.nonce(L.ALG_AESGCM, n), ad, pt):
                    raise AssertionError(f"seal mismatch t={t} j={j}")
                if j % 5 == 2:
                    bad = bytearray(ct)
                    bad[int(r.integers(0, len(bad)))] ^= 1 << int(r.integers(0, 8))
                    try:
                        cs.DecryptDanger(None, ad, bytes(bad), n)
                        raise AssertionError(f"forgery accepted t={t} j={j}")
                    except ErrOpen:
                        pass
                elif cs.DecryptDanger(None, ad, ct, n).bytes() != pt:
                    raise AssertionError(f"open mismatch t={t} j={j}")
        except Exception as ex:
            errors.append(ex)

    ths = [threading.Thread(target=worker, args=(t,)) for t in range(24)]
    before = engine.stats()
    try:
        for th in ths:
            th.start()
        for th in ths:
            th.join()
        assert not errors, errors[:3]
        after = engine.stats()
        # every call counted once, alone or combined (neb_engine_stats / neb_engine_pkt_combined)
        assert after["pkt_calls"] - before["pkt_calls"] >= 24 * 120 * 2
        combined = after["pkt_combined_calls"] - before["pkt_combined_calls"]
        launches = after["pkt_combined_launches"] - before["pkt_combined_launches"]
        assert combined >= launches >= 0 and combined <= 32 * launches
        print(f"combined {combined} calls in {launches} launches")
    finally:
        for cs, _ in states:
            cs.destroy()
