"""GPU: directed tests of the authenticators, every kernel path bit-exact against the CPU oracle.

A. The Poly1305 edge vectors (tests/poly1305_ref.py, tests/golden/poly1305_edges.json: accumulator
   values where p5_finish's conditional subtract and the carries of h + s matter) through the
   ChaCha batch kernel, one and four copies of each, and through the per-packet kernel, against
   the committed bytes.
B. The block-count sweep (tests/auth_cases.py) through the 64-lane tail kernel, the single-key
   kernel (whole passes, and a partial last pass), the mixed-key chunks at 4, 8 and 16 lanes per
   packet (the widths asserted on the scheduler model's plan of the same descriptors), the ChaCha
   batch kernel and the per-packet kernels of both ciphers.
C. The forgery matrix through the same paths: statuses and the whole arena equal the oracle's
   opening of the same tampered arena, so a failed packet's dst[0:len) is zero and nothing else
   has changed, in place and out of place.
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import auth_cases as A  # noqa: E402
import poly1305_ref as R  # noqa: E402
from nebula_amd import _lib as L  # noqa: E402
from nebula_amd import noiseutil as N  # noqa: E402
from nebula_amd import workload as W  # noqa: E402
from test_gpu_parity import oracle_open, oracle_seal, run_device  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL_BATCH = 6144   # aes_gcm.hip kSmallBatch: up to here one key's batch runs in the tail kernel
SINGLE_PPW = 16      # aes_gcm.hip kPpw: packets per wave of the single-key kernel
SINGLE_WAVES = 16    # aes_gcm.hip kSingleWaves: waves per workgroup


def _seal_open_vs_oracle(engine, b, ref, ref_o):
    got, st = run_device(engine, b, seal=True)
    assert (st == 0).all()
    _assert_same(got, ref, b)
    got_o, st_o = run_device(engine, b, seal=False, arena=ref)
    assert (st_o == 0).all()
    _assert_same(got_o, ref_o, b)


def _assert_same(got, exp, b):
    """Arenas equal; on a mismatch name the first packet whose slot differs and its shape."""
    if np.array_equal(got, exp):
        return
    pos = int(np.flatnonzero(got != exp)[0])
    order = np.argsort(b.desc["aad_off"], kind="stable")
    i = int(order[max(int(np.searchsorted(b.desc["aad_off"][order], pos, side="right")) - 1, 0)])
    d = b.desc[i]
    raise AssertionError(f"arena differs at byte {pos}: packet {i}, aad_len {d['aad_len']} (na "
                         f"{(int(d['aad_len']) + 15) // 16}), len {d['len']} (m {(int(d['len']) + 15) // 16}), "
                         f"key {d['key_id']}, {int((got != exp).sum())} bytes differ in all")


def _refs(oracle_mod, b):
    ref, st = oracle_seal(oracle_mod, b)
    ref_o, st_o = oracle_open(oracle_mod, b, ref)
    assert (st == 0).all() and (st_o == 0).all()
    return ref, ref_o


# ---- A: Poly1305 edge vectors ------------------------------------------------------------------

def _vectors():
    with open(os.path.join(GOLD, "poly1305_edges.json")) as f:
        return json.load(f)


def _vector_batch(vecs, copies):
    """Each vector `copies` times in consecutive slots of its own (a wave holds 4 packets): the
    plaintext batch over the two keys, the sealed arena by the committed bytes, the opened one."""
    rng = np.random.default_rng(1305)
    keys = [k.hex() for k in R.KEYS]
    n = len(vecs) * copies
    stride = 768
    arena = rng.integers(0, 256, n * stride, dtype=np.uint8)
    sealed = arena.copy()
    desc = np.zeros(n, L.DESC_DTYPE)
    for i in range(n):
        v = vecs[i // copies]
        aad, pt, ct = (np.frombuffer(bytes.fromhex(v[k]), np.uint8) for k in ("aad", "plaintext", "sealed"))
        base, src = i * stride, i * stride + (len(aad) + 15) // 16 * 16
        assert src + len(ct) <= base + stride
        for a in (arena, sealed):
            a[base:base + len(aad)] = aad
        arena[src:src + len(pt)] = pt
        sealed[src:src + len(ct)] = ct
        desc[i] = (src, src, base, v["counter"], len(pt), len(aad), keys.index(v["key"]), 0)
    opened = sealed.copy()
    for i in range(n):
        s, ln = int(desc["src_off"][i]), int(desc["len"][i])
        opened[s:s + ln] = arena[s:s + ln]
    kb = np.frombuffer(b"".join(R.KEYS), np.uint8).copy()
    return W.Batch(L.ALG_CHACHAPOLY, kb, np.zeros(2, np.uint32), desc, arena, stride, "poly1305-edges"), sealed, opened


@pytest.mark.parametrize("copies", [1, 4])
def test_poly1305_edge_vectors_batch(engine, copies):
    """All 34 vectors in one batch with two keys through the ChaCha batch kernel: the arena equals
    the committed sealed bytes (oracle == EVP == the Python helper) and opens back, every status 0.
    copies = 4: one wave holds four packets at the same edge."""
    vecs = _vectors()
    assert len(vecs) == 34
    b, sealed, opened = _vector_batch(vecs, copies)
    assert set(b.desc["key_id"]) == {0, 1}
    got, st = run_device(engine, b, seal=True)
    for i in np.flatnonzero([not np.array_equal(got[i * b.stride:(i + 1) * b.stride],
                                                sealed[i * b.stride:(i + 1) * b.stride]) for i in range(b.n)]):
        v = vecs[i // copies]
        raise AssertionError(f"sealed bytes differ: {v['shape']}/{v['target']} (copy {i % copies})")
    assert (st == 0).all()
    got_o, st_o = run_device(engine, b, seal=False, arena=sealed)
    bad = np.flatnonzero(st_o != 0)
    assert len(bad) == 0, [f"{vecs[i // copies]['shape']}/{vecs[i // copies]['target']}" for i in bad]
    assert np.array_equal(got_o, opened)


def test_poly1305_edge_vectors_per_packet(engine):
    """The same vectors through EncryptDanger / DecryptDanger (chacha_one_kernel)."""
    ciphers = {k.hex(): N.CipherChaChaPoly.Cipher(engine, k) for k in R.KEYS}
    try:
        for v in _vectors():
            aad, pt, sealed = (bytes.fromhex(v[k]) for k in ("aad", "plaintext", "sealed"))
            assert (len(aad) + 15) // 16 * 16 + len(sealed) <= 2048  # fits the kernel's argument block
            cs = ciphers[v["key"]]
            assert cs.EncryptDanger(None, aad, pt, v["counter"]).bytes() == sealed, (v["shape"], v["target"])
            assert cs.DecryptDanger(None, aad, sealed, v["counter"]).bytes() == pt, (v["shape"], v["target"])
    finally:
        for cs in ciphers.values():
            cs.destroy()


# ---- B: block-count sweep ----------------------------------------------------------------------

def test_sweep_single_key_tail_kernel(engine, oracle_mod):
    """One key, the 1407 shapes: at most kSmallBatch packets, so the 64-lane tail kernel
    (GhShoup64) takes them all."""
    b = A.shapes_batch(L.ALG_AESGCM, A.grid(), 0, seed=64, nkeys=1)
    assert b.n == 1407 <= SMALL_BATCH and A.lane_conditions(A.desc_shapes(b.desc), 64) == []
    _seal_open_vs_oracle(engine, b, *_refs(oracle_mod, b))


_SINGLE = {}


@pytest.mark.parametrize("max_grid", [0, 4])
def test_sweep_single_key_kernel(engine, oracle_mod, knobs, max_grid):
    """One key, five copies of the 1407 shapes with fresh contents (7035 > kSmallBatch): the
    single-key kernel at 4 lanes per packet (GhFullPerm). max_grid = 4 caps its grid at 64 waves,
    so 6 whole passes run there and the last 56 of the 440 groups in the 64-lane tail kernel."""
    if not _SINGLE:
        b = A.shapes_batch(L.ALG_AESGCM, A.grid(), 0, seed=4, copies=5, nkeys=1)
        _SINGLE.update(b=b, refs=_refs(oracle_mod, b))
    b = _SINGLE["b"]
    assert b.n == 7035 > SMALL_BATCH and A.lane_conditions(A.desc_shapes(b.desc), 4) == []
    if max_grid:
        knobs(L.KNOB_SINGLE_MAX_GRID, max_grid)
        groups, slots = -(-b.n // SINGLE_PPW), max_grid * SINGLE_WAVES
        assert groups > slots and groups % slots  # a partial last pass
    _seal_open_vs_oracle(engine, b, *_SINGLE["refs"])


@pytest.mark.parametrize("lg", [2, 3, 4])
def test_sweep_mixed_key_chunks(engine, oracle_mod, lg):
    """One key per shape with 16, 7 or 3 packets of it: front chunks at 4 lanes per packet
    (GhChunk4), leftover chunks at 8 and at 16 (GhChunkTail). The widths are not guessed: the
    scheduler model plans these descriptors, every packet with at least min_blocks(lg) blocks is
    at 2^lg lanes (shorter size classes are capped narrower: class 0, n <= 4, at 4 lanes and
    class 1, n <= 8, at 8), and the packets at that width meet the lane conditions."""
    b = A.shapes_batch(L.ALG_AESGCM, A.mixed_grid(lg), A.PER_KEY[lg], seed=lg)
    assert b.nkeys < 8192
    got, front = A.planned(b.desc)
    shapes = A.desc_shapes(b.desc)
    wide = shapes.sum(axis=1) + 1 >= A.min_blocks(lg)
    assert (got[wide] == lg).all() and (front[wide] == (lg == 2)).all() and (got[~wide] < lg).all()
    assert A.lane_conditions(shapes[got == lg], 1 << lg) == []
    _seal_open_vs_oracle(engine, b, *_refs(oracle_mod, b))


def test_sweep_chacha_batch_kernel(engine, oracle_mod):
    """The 1407 shapes over two keys: every AAD phase phi with every last lane, whole-wave fast
    rounds beside slow ones in one wave."""
    b = A.shapes_batch(L.ALG_CHACHAPOLY, A.grid(), 0, seed=20, nkeys=2)
    assert A.chacha_conditions(A.desc_shapes(b.desc)) == []
    _seal_open_vs_oracle(engine, b, *_refs(oracle_mod, b))


@pytest.mark.parametrize("cf", [N.CipherAESGCM, N.CipherChaChaPoly], ids=["AESGCM", "ChaChaPoly"])
def test_sweep_per_packet_kernels(engine, oracle_mod, cf):
    """na in {0, 1, 2, 5, 16, 17} with every m of the grid (all fit the 2048-byte argument block)
    through EncryptDanger / DecryptDanger: gcm_one_kernel at 64 lanes, chacha_one_kernel."""
    rng = np.random.default_rng(2048 + cf.alg)
    key = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    cs = cf.Cipher(engine, key)
    try:
        for na, m, al, ln in A.grid((0, 1, 2, 5, 16, 17)):
            assert 16 * na + ln + 16 <= 2048
            aad = bytes(rng.integers(0, 256, al, dtype=np.uint8))
            pt = bytes(rng.integers(0, 256, ln, dtype=np.uint8))
            ctr = int(rng.integers(0, 2**62))
            exp = oracle_mod.seal(cf.alg, key, oracle_mod.nonce(cf.alg, ctr), aad, pt)
            assert cs.EncryptDanger(None, aad, pt, ctr).bytes() == exp, (na, m, al, ln)
            assert cs.DecryptDanger(None, aad, exp, ctr).bytes() == pt, (na, m, al, ln)
    finally:
        cs.destroy()


# ---- C: forgery matrix -------------------------------------------------------------------------

def _run_forgery(engine, oracle_mod, f):
    sealed, st = oracle_seal(oracle_mod, f.sealed)
    assert (st == 0).all()
    t = f.tamper(sealed)
    ob = f.open_batch()
    exp, st_exp = oracle_open(oracle_mod, ob, t)
    victims = sorted(f.victims)
    assert np.flatnonzero(st_exp).tolist() == victims and (st_exp[victims] == L.STATUS_AUTH_FAILED).all()
    got, st = run_device(engine, ob, seal=False, arena=t)
    wrong = np.flatnonzero(st != st_exp)
    assert len(wrong) == 0, [(int(i), f.victims.get(int(i), "clean"), int(ob.desc["len"][i])) for i in wrong]
    for i in victims:
        d = ob.desc[i]
        lo, hi = i * A.FORGE_STRIDE, (i + 1) * A.FORGE_STRIDE
        dst, ln = int(d["dst_off"]), int(d["len"])
        assert not got[dst:dst + ln].any(), (i, f.victims[i], "dst not wiped")
        if ln == 0:  # nothing to wipe: no byte changes at all
            assert np.array_equal(got[lo:hi], t[lo:hi]), (i, f.victims[i])
        elif dst != int(d["src_off"]):  # out of place: only dst[0:len) differs from the input
            same = np.ones(hi - lo, bool)
            same[dst - lo:dst - lo + ln] = False
            assert np.array_equal(got[lo:hi][same], t[lo:hi][same]), (i, f.victims[i], "wrote outside dst")
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, (int(bad[0]) // A.FORGE_STRIDE, f.victims.get(int(bad[0]) // A.FORGE_STRIDE, "clean"),
                           int(bad[0]) % A.FORGE_STRIDE, len(bad))


def _one_key(ln):
    return np.zeros(len(ln), np.int64)


def test_forgery_single_key_tail_kernel(engine, oracle_mod):
    _run_forgery(engine, oracle_mod, A.forgery_case(L.ALG_AESGCM, _one_key, 1, seed=640))


def test_forgery_single_key_kernel(engine, oracle_mod):
    """The matrix, then clean 100-byte packets up to 6160: past kSmallBatch, one whole pass of the
    single-key kernel and no tail."""
    f = A.forgery_case(L.ALG_AESGCM, _one_key, 1, seed=40, filler_lens=[100] * (6160 - A.FORGE_N))
    assert f.sealed.n == 6160 > SMALL_BATCH
    _run_forgery(engine, oracle_mod, f)


def test_forgery_chacha_batch_kernel(engine, oracle_mod):
    _run_forgery(engine, oracle_mod, A.forgery_case(L.ALG_CHACHAPOLY, lambda ln: np.arange(len(ln)) % 2, 2, seed=20))


@pytest.mark.parametrize("lg", [2, 3, 4])
def test_forgery_mixed_key_chunks(engine, oracle_mod, lg):
    """Keys of 16, 7 or 3 packets of one length each (clean packets fill the last key of a
    length), so every packet long enough runs at 2^lg lanes; which ones did is read from the
    scheduler model's plan. Payloads of 1 and 17 bytes are size class 0 and stay at 4 lanes, so
    the matrix runs at all five rotations of its length cycle: over them every victim kind is
    opened at 2^lg lanes, with 0-, 100- and 1300-byte payloads among them."""
    kinds, lens = set(), set()
    for rot in range(5):
        f = A.mixed_forgery_case(L.ALG_AESGCM, lg, rot)
        got, _ = A.planned(f.sealed.desc)
        assert (got[A.desc_shapes(f.sealed.desc).sum(axis=1) + 1 >= A.min_blocks(lg)] == lg).all()
        kinds |= {k for i, k in f.victims.items() if got[i] == lg}
        lens |= {int(f.sealed.desc["len"][i]) for i in f.victims if got[i] == lg}
        _run_forgery(engine, oracle_mod, f)
    assert kinds == set(A.KINDS) and lens >= {0, 100, 1300}
