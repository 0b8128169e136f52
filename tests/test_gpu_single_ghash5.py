"""The single-key kernel's Horner multiply (gf_mul_full5: 5-bit GHASH windows read with
ds_read_b64) through the C ABI against the oracle, bit-exact.

One key with key_hint set and 6160 packets per batch: just over kSmallBatch = 6144, below which the
tail kernel takes the whole batch and gcm_single_kernel never runs. Three shapes: payload lengths
around every block boundary with a 16-byte AAD, the relay shape (1348-byte AAD, empty payload:
rounds that are GHASH only), and 4112-byte payloads (the 2^16 counter tier). Each is sealed and
compared byte for byte (tags included), opened back, and opened with one tag byte flipped."""
import numpy as np
import pytest

from nebula_amd import _lib as L
from nebula_amd import workload as W

from test_gpu_parity import oracle_open, oracle_seal, run_device

pytestmark = pytest.mark.gpu

N = 6160
LENS = (0, 1, 15, 16, 17, 31, 33, 63, 64, 65, 79, 80, 81, 127, 129, 200)
SHAPES = {
    "lens": lambda: W.make_batch(L.ALG_AESGCM, N, 1, sizes=LENS, ratio=(1,) * len(LENS), seed=0x6A55, name="ghash5"),
    "relay": lambda: W.relay_batch(L.ALG_AESGCM, N, 1, aad_len=1348, seed=0x6A56),
    "tier16": lambda: W.make_batch(L.ALG_AESGCM, N, 1, sizes=(4112,), seed=0x6A57, name="ghash5-4112"),
}
_CACHE = {}


def _case(oracle_mod, shape):
    """The batch, its oracle-sealed arena and the oracle's opening of it: computed once per shape."""
    if shape not in _CACHE:
        b = SHAPES[shape]()
        assert b.n == N > 6144 and b.nkeys == 1
        ref, st = oracle_seal(oracle_mod, b)
        assert (st == 0).all()
        ref_o, st_o = oracle_open(oracle_mod, b, ref)
        assert (st_o == 0).all()
        _CACHE[shape] = (b, ref, ref_o)
    return _CACHE[shape]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_seal_matches_oracle(engine, oracle_mod, shape):
    b, ref, _ = _case(oracle_mod, shape)
    if shape == "lens":
        assert sorted(set(b.desc["len"].tolist())) == sorted(LENS)
    got, st = run_device(engine, b, seal=True)
    assert (st == 0).all()
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_open_restores_plaintext(engine, oracle_mod, shape):
    b, ref, ref_o = _case(oracle_mod, shape)
    got, st = run_device(engine, b, seal=False, arena=ref)
    assert (st == 0).all()
    assert np.array_equal(got, ref_o)
    d = b.desc
    used = np.arange(b.stride)[None, :] < (d["src_off"] - d["aad_off"] + d["len"])[:, None].astype(np.int64)
    assert np.array_equal(got.reshape(N, b.stride)[used], b.arena.reshape(N, b.stride)[used])


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_flipped_tag_byte_fails_that_packet_alone(engine, oracle_mod, shape):
    b, ref, _ = _case(oracle_mod, shape)
    victim = 3001
    bad = ref.copy()
    bad[int(b.desc["src_off"][victim]) + int(b.desc["len"][victim]) + 9] ^= 0x20
    _, st = run_device(engine, b, seal=False, arena=bad)
    assert st[victim] == L.STATUS_AUTH_FAILED
    assert (np.delete(st, victim) == 0).all()
