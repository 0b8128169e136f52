"""CPU model of the single-key kernel's 5-bit window GHASH multiply (gf_mul_full5):
the table F5[P][v] = (v·x^5P)·H^4 derived from the key record's nibble table exactly as the kernel
prologue derives it, laid out in LDS as two 256-byte rows of 8-byte halves per window, and the
window extraction of the multiply (shifts, and an alignbit for the windows that straddle two
words). The XOR of the 26 looked-up entries must be x·H^4, and every row must be one conflict-free
ds_read_b64 table (32 entries on 32 disjoint bank pairs covering the 64 banks)."""
import random

import pytest

NWIN = 26  # 128 = 25·5 + 3
M32 = 0xFFFFFFFF


def coeff(b):
    """x^b as a 16-byte block (GCM bit order: x^0 is the MSB of byte 0)."""
    e = bytearray(16)
    e[b // 8] |= 0x80 >> (b % 8)
    return bytes(e)


def nibble_elem(p, v):
    """nibble v at nibble position p: v's MSB is x^(4p)."""
    e = bytearray(16)
    for t in range(4):
        if (v >> (3 - t)) & 1:
            b = 4 * p + t
            e[b // 8] |= 0x80 >> (b % 8)
    return bytes(e)


def record_single_bits(ora, H4):
    """The entries of the record's nibble table F_p[v] = (v·x^4p)·H^4 that the prologue reads:
    F_(b/4)[8 >> (b%4)] for b < 128, keyed (p, v)."""
    return {(b // 4, 8 >> (b % 4)): ora.gf128_mul(nibble_elem(b // 4, 8 >> (b % 4)), H4) for b in range(128)}


def build_f5_lds(rec):
    """The 13 KiB LDS image: thread t < 832 takes (P, v) = (t / 32, t % 32), XORs the products of
    the coefficients x^(5P+j) that bit 4-j of v selects, and stores words 0-1 at (2P)·256 + 8v and
    words 2-3 at (2P+1)·256 + 8v."""
    lds = bytearray(2 * NWIN * 256)
    for t in range(NWIN * 32):
        P, v = t // 32, t % 32
        acc = 0
        for j in range(5):
            b = 5 * P + j
            bc = min(b, 127)
            c = int.from_bytes(rec[(bc // 4, 8 >> (bc % 4))], "big")
            if b < 128 and (v >> (4 - j)) & 1:
                acc ^= c
        e = acc.to_bytes(16, "big")
        lds[(2 * P) * 256 + 8 * v:(2 * P) * 256 + 8 * v + 8] = e[:8]
        lds[(2 * P + 1) * 256 + 8 * v:(2 * P + 1) * 256 + 8 * v + 8] = e[8:]
    return lds


def window_addr(xw, P):
    """The table address (v << 3) of window P from the 4 big-endian words, as the kernel forms it."""
    q, r = (5 * P) >> 5, (5 * P) & 31
    if r > 27 and q < 3:  # straddles words q and q+1: v_alignbit
        w = (((xw[q] << 32) | xw[q + 1]) >> (56 - r)) & M32
    elif r <= 24:
        w = xw[q] >> (24 - r)
    else:
        w = (xw[q] << (r - 24)) & M32
    return w & 0xF8


def mul_full5(lds, x):
    xw = [int.from_bytes(x[4 * q:4 * q + 4], "big") for q in range(4)]
    lo = hi = 0
    for P in range(NWIN):
        a = window_addr(xw, P)
        lo ^= int.from_bytes(lds[(2 * P) * 256 + a:(2 * P) * 256 + a + 8], "big")
        hi ^= int.from_bytes(lds[(2 * P + 1) * 256 + a:(2 * P + 1) * 256 + a + 8], "big")
    return lo.to_bytes(8, "big") + hi.to_bytes(8, "big")


EDGE_BITS = [0, 4, 5] + list(range(29, 36)) + list(range(59, 66)) + list(range(94, 101)) + list(range(124, 128))


def test_window_extraction_covers_every_coefficient_once():
    """Coefficient x^b lands in window b/5 at bit 4 - b%5 of its value, and nowhere else."""
    for b in range(128):
        x = coeff(b)
        xw = [int.from_bytes(x[4 * q:4 * q + 4], "big") for q in range(4)]
        for P in range(NWIN):
            want = (1 << (4 - b % 5)) << 3 if P == b // 5 else 0
            assert window_addr(xw, P) == want, (b, P)
    ones = [M32] * 4
    assert [window_addr(ones, P) for P in range(NWIN)] == [0xF8] * 25 + [0xE0]  # window 25: three bits << 2


def test_random_pairs(oracle_mod):
    rng = random.Random(0x6A5)
    for _ in range(1000):
        H4 = bytes(rng.getrandbits(8) for _ in range(16))
        x = bytes(rng.getrandbits(8) for _ in range(16))
        lds = build_f5_lds(record_single_bits(oracle_mod, H4))
        assert mul_full5(lds, x) == oracle_mod.gf128_mul(x, H4)


@pytest.fixture(scope="module")
def fixed_table(oracle_mod):
    rng = random.Random(55)
    H4 = bytes(rng.getrandbits(8) for _ in range(16))
    return H4, build_f5_lds(record_single_bits(oracle_mod, H4))


def test_record_entries_are_the_nibble_table(oracle_mod, fixed_table):
    """The 128 entries read are those of the full nibble table (32 positions × 16 values): every
    entry of that table is the XOR of the single-coefficient entries of its set bits."""
    H4, _ = fixed_table
    rec = record_single_bits(oracle_mod, H4)
    for p in range(32):
        for v in range(16):
            acc = 0
            for t in range(4):
                if (v >> (3 - t)) & 1:
                    acc ^= int.from_bytes(rec[(p, 8 >> t)], "big")
            assert acc.to_bytes(16, "big") == oracle_mod.gf128_mul(nibble_elem(p, v), H4)


@pytest.mark.parametrize("b", EDGE_BITS)
def test_single_coefficients(oracle_mod, fixed_table, b):
    H4, lds = fixed_table
    assert mul_full5(lds, coeff(b)) == oracle_mod.gf128_mul(coeff(b), H4)


def test_all_ones_and_zero(oracle_mod, fixed_table):
    H4, lds = fixed_table
    assert mul_full5(lds, b"\xff" * 16) == oracle_mod.gf128_mul(b"\xff" * 16, H4)
    assert mul_full5(lds, bytes(16)) == bytes(16)


def test_rows_are_conflict_free_b64_tables():
    """A ds_read_b64 banks on (addr/4) mod 64: the 32 entries of every row sit on 32 disjoint bank
    pairs that together cover all 64 banks, so any 32 lanes read a row without a conflict."""
    assert 2 * NWIN * 256 == 13 * 1024
    for row in range(2 * NWIN):
        pairs = []
        for v in range(32):
            addr = row * 256 + 8 * v
            assert addr % 8 == 0 and addr < 65536  # aligned, inside the ds_read offset field
            pairs.append(((addr // 4) % 64, (addr // 4 + 1) % 64))
        banks = [b for pr in pairs for b in pr]
        assert len(set(banks)) == 64 and sorted(banks) == list(range(64))
