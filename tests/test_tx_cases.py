"""CPU: the directed transmit cases (tests/tx_cases.py) reach every condition the transmit kernels
branch on, every steered checksum really is a computed zero, and every segment the oracle makes of
them passes a verifier written from the RFCs (791, 768, 9293, 8200, 1071) and the virtio NEEDS_CSUM
rule, with a bytewise sum of its own and none of the oracle's helpers."""
import struct

import pytest

import segment_oracle as S
import tx_cases as T


@pytest.fixture(scope="module")
def cases():
    return T.cases()


@pytest.fixture(scope="module")
def reached(cases):
    return {name: T.conditions({name: reads}) for name, reads in cases.items()}


def test_every_condition_is_reached(cases):
    assert len(set(T.required())) == len(T.required())
    assert T.uncovered(cases) == []


def test_every_case_reaches_something_of_its_own(cases, reached):
    """A case that could be removed without uncovering a condition is listed in REDUNDANT with its
    reason, or it goes."""
    req = set(T.required())
    assert all(name in cases and why for name, why in T.REDUNDANT)
    for name in cases:
        rest = set().union(*(c for n, c in reached.items() if n != name))
        if name in dict(T.REDUNDANT):
            assert not (req - rest), name
        else:
            assert req - rest, f"{name} reaches nothing of its own"


def test_batch_limits_and_skews(cases):
    reads, _ = T.batch(cases, 3, 0)
    assert sum(len(p["data"]) for p in reads) <= 1 << 20
    nw = sum(len(T.read_result(p)[1]) for p in reads)
    assert 300 <= nw <= 2500 and nw % 256 != 0
    seen = {}
    for rot in T.ROTATIONS:
        _, skews = T.batch(cases, 3, rot)
        assert set(skews) == set(range(16))
        it = iter(skews)
        for name, rs in cases.items():
            mine = {next(it) for _ in rs}
            seen.setdefault(name, set()).update(mine)
            if len(rs) >= 4:
                assert len(mine) >= 4 and any(s & 1 for s in mine), name
    for name, s in seen.items():
        assert len(s) >= 4 and any(x & 1 for x in s), name


def test_steered_checksums_are_computed_zeros(cases):
    n = 0
    for name in ("zero_udp4", "zero_udp6", "zero_tcp4", "zero_tcp6"):
        pk = cases[name][0]
        st, segs = T.read_result(pk)
        assert st == S.OK and len(segs) == 4
        f = T.field_of(pk)
        for j in (0, 1, 3):
            cs = pk["csum_start"]
            assert _ones_zero(_sum_be(_zeroed(segs[j], f)[cs:]) + _pseudo(segs[j], cs))  # ~sum = 0 with the field zeroed
            assert T.computed_l4(pk, segs[j]) == 0
            assert segs[j][f:f + 2] == (b"\xff\xff" if "udp" in name else b"\0\0"), (name, j)
            n += 1
        assert T.computed_l4(pk, segs[2]) != 0  # the segment that was not steered
    for pk in cases["zero_finish"]:
        seg = T.read_result(pk)[1][0]
        f = T.field_of(pk)
        assert T.computed_l4(pk, seg) == 0
        assert seg[f:f + 2] == (b"\xff\xff" if pk["csum_offset"] == 6 else b"\0\0")
        n += 1
    assert n == 15
    for pk, j in zip(cases["zero_ip_header"], (1, 0)):
        seg = T.read_result(pk)[1][j]
        assert seg[10:12] == b"\0\0" and _sum_be(seg[:(seg[0] & 15) * 4]) % 0xFFFF == 0


# ---- the verifier -----------------------------------------------------------------------------

def _sum_be(b):
    """Σ of big-endian 16-bit words, an odd last byte as a high byte; not folded."""
    return sum(x << 8 if i % 2 == 0 else x for i, x in enumerate(b))


def _ones_zero(s):
    """The one's-complement sum s is a zero: 0xFFFF after end-around carries (or all zero bits)."""
    return s % 0xFFFF == 0


def _zeroed(seg, f):
    return seg[:f] + b"\0\0" + seg[f + 2:]


def _pseudo(seg, cs):
    """RFC 9293 3.1 / RFC 768 / RFC 8200 8.1: addresses, zero + protocol, the L4 length."""
    v4 = seg[0] >> 4 == 4
    proto = 6 if _proto(seg) == "tcp" else 17
    return _sum_be(seg[12:20] if v4 else seg[8:40]) + proto + len(seg) - cs


def _proto(seg):
    # the builders' protocol: IPv4's field, or IPv6's next header behind at most one extension header
    nh = seg[9] if seg[0] >> 4 == 4 else seg[6] if seg[6] != 60 else seg[40]
    return {6: "tcp", 17: "udp"}[nh]


def verify_read(pk, segs):
    d, cs, gso = pk["data"], pk["csum_start"], pk["gso_size"]
    kind = T.kind_of(pk)
    if kind == "pass":
        assert segs == [d]
        return
    if kind == "finish":
        (seg,), f = segs, cs + pk["csum_offset"]
        assert len(seg) == len(d) and _zeroed(seg, f) == _zeroed(d, f)
        # the field held a partial sum; the result makes [cs, len) plus that partial sum to zero
        total = _sum_be(_zeroed(seg, f)[cs:]) + struct.unpack_from(">H", d, f)[0] + struct.unpack_from(">H", seg, f)[0]
        assert _ones_zero(total) and total != 0
        if pk["csum_offset"] == 6:
            assert seg[f:f + 2] != b"\0\0"
        return
    v4 = d[0] >> 4 == 4
    hl = cs + (8 if kind == "udp" else (d[cs + 12] >> 4) * 4)
    pay = d[hl:]
    assert len(segs) == max(1, -(-len(pay) // gso))
    assert b"".join(s[hl:] for s in segs) == pay
    id0, = struct.unpack_from(">H", d, 4)
    for j, seg in enumerate(segs):
        last = j == len(segs) - 1
        assert len(seg) - hl == (gso if not last else len(pay) - j * gso)
        changed = set()
        if v4:
            ihl = (seg[0] & 15) * 4
            assert struct.unpack_from(">H", seg, 2)[0] == len(seg)
            assert struct.unpack_from(">H", seg, 4)[0] == (id0 + j) % 65536
            assert _ones_zero(_sum_be(seg[:ihl]))                    # RFC 791: the header sums to zero
            assert seg[10:12] != b"\xff\xff"                         # ~s of a non-zero s is never all ones
            changed |= {2, 3, 4, 5, 10, 11}
        else:
            assert struct.unpack_from(">H", seg, 4)[0] == len(seg) - 40
            changed |= {4, 5}
        if kind == "tcp":
            (seq0,), fl0 = struct.unpack_from(">I", d, cs + 4), d[cs + 13]
            assert struct.unpack_from(">I", seg, cs + 4)[0] == (seq0 + j * gso) % (1 << 32)
            want = fl0 & ~((0 if j == 0 else T.CWR) | (0 if last else T.FIN | T.PSH))
            assert seg[cs + 13] == want
            f = cs + 16
            assert seg[f:f + 2] != b"\xff\xff"
            changed |= {cs + 4, cs + 5, cs + 6, cs + 7, cs + 13}
        else:
            assert struct.unpack_from(">H", seg, cs + 4)[0] == len(seg) - cs
            f = cs + 6
            assert seg[f:f + 2] != b"\0\0"                           # RFC 768: zero means "no checksum"
            changed |= {cs + 4, cs + 5}
        changed |= {f, f + 1}
        assert _ones_zero(_sum_be(seg[cs:]) + _pseudo(seg, cs))
        assert all(seg[i] == d[i] for i in range(hl) if i not in changed), j


def test_oracle_segments_pass_an_independent_verifier(cases):
    nseg = nrefused = 0
    for name, reads in cases.items():
        for pk in reads:
            st, segs = T.read_result(pk)
            if st != S.OK:
                nrefused += 1
                continue
            verify_read(pk, segs)
            nseg += len(segs)
    assert nseg > 300 and nrefused == 14


def test_the_verifier_notices_a_wrong_segment(cases):
    """The verifier is no rubber stamp: one flipped bit in a checksum, an ID, a sequence number, a
    flag byte, a length or a payload byte fails it."""
    pk = T.tso(4, T.rand_bytes(1000, 1), 400, flags=0xFF)
    segs = T.read_result(pk)[1]
    verify_read(pk, segs)
    for j, off in ((0, 36), (1, 5), (2, 27), (1, 33), (0, 33), (1, 3), (2, 50), (0, 11), (1, 8)):
        bad = list(segs)
        bad[j] = segs[j][:off] + bytes([segs[j][off] ^ 1]) + segs[j][off + 1:]
        with pytest.raises(AssertionError):
            verify_read(pk, bad)
