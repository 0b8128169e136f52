"""ChaCha20-Poly1305 (RFC 8439) in plain Python integers, and directed Poly1305 edge vectors.

Standard library only. The ChaCha20 block function, Nebula's one-time key (nonce
00000000 || LE64(counter), chachapoly.go:30-34), Poly1305 over the AEAD layout
AAD | pad | CT | pad | LE64(aad_len) | LE64(len), and solve(): given a key, the packet is built so
that the accumulator h = Poly1305's sum reduced into [0, p), before the final `+ s`, is a chosen
value. Random data reaches the values where the final reduction matters (h below 5, h next to p,
h next to 2^128, a carry through all four words of h + s) with probability about 2^-128; here
the last AAD block (relay shape) or the last ciphertext block (data shape) is solved for them.

With r and s known, h = (... (h_prev + b + 2^128)·r + L + 2^128)·r for the solved block b and the
length block L, so b = (T·r^-1 - L - 2^128)·r^-1 - h_prev - 2^128 (mod p). b must be below 2^128 to
be a block, which holds for about one counter in four; solve() walks the counters until it does.

EDGE_TARGETS names the 16 targets; vectors() makes the 34 committed vectors
(tests/golden/poly1305_edges.json, written by make_golden.py with the sealed bytes the oracle and
OpenSSL EVP agree on).
"""
import hashlib
import struct

P = (1 << 130) - 5
M128 = (1 << 128) - 1
CLAMP = 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
MAX_COUNTER = 200


def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & 0xFFFFFFFF


def _qr(x, a, b, c, d):
    x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & 0xFFFFFFFF; x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & 0xFFFFFFFF; x[b] = _rotl(x[b] ^ x[c], 7)


def chacha20_block(key: bytes, block_counter: int, nonce: bytes) -> bytes:
    """RFC 8439 §2.3: the 64-byte keystream block."""
    assert len(key) == 32 and len(nonce) == 12
    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574]
    init += struct.unpack("<8I", key) + (block_counter & 0xFFFFFFFF,) + struct.unpack("<3I", nonce)
    x = list(init)
    for _ in range(10):
        _qr(x, 0, 4, 8, 12); _qr(x, 1, 5, 9, 13); _qr(x, 2, 6, 10, 14); _qr(x, 3, 7, 11, 15)
        _qr(x, 0, 5, 10, 15); _qr(x, 1, 6, 11, 12); _qr(x, 2, 7, 8, 13); _qr(x, 3, 4, 9, 14)
    return struct.pack("<16I", *[(a + b) & 0xFFFFFFFF for a, b in zip(x, init)])


def nebula_nonce(counter: int) -> bytes:
    return b"\0\0\0\0" + struct.pack("<Q", counter)


def one_time_key(key: bytes, nonce: bytes):
    """RFC 8439 §2.6: (r clamped, s) from ChaCha20 block 0."""
    b0 = chacha20_block(key, 0, nonce)
    return int.from_bytes(b0[:16], "little") & CLAMP, int.from_bytes(b0[16:32], "little")


def keystream(key: bytes, nonce: bytes, nbytes: int) -> bytes:
    """The payload's keystream: ChaCha20 blocks 1, 2, ..."""
    out = b"".join(chacha20_block(key, 1 + i, nonce) for i in range((nbytes + 63) // 64))
    return out[:nbytes]


def xor(a: bytes, b: bytes) -> bytes:
    return bytes(x ^ y for x, y in zip(a, b))


def mac_data(aad: bytes, ct: bytes) -> bytes:
    """RFC 8439 §2.8: what Poly1305 runs over."""
    return (aad + b"\0" * (-len(aad) % 16) + ct + b"\0" * (-len(ct) % 16) +
            struct.pack("<QQ", len(aad), len(ct)))


def accumulate(r: int, data: bytes, h: int = 0) -> int:
    """Poly1305's accumulator over data (RFC 8439 §2.5.1), reduced into [0, p): the value the
    final `+ s` is applied to."""
    for i in range(0, len(data), 16):
        blk = data[i:i + 16]
        h = (h + int.from_bytes(blk, "little") + (1 << (8 * len(blk)))) * r % P
    return h


def tag_of(h: int, s: int) -> bytes:
    return ((h + s) & M128).to_bytes(16, "little")


def seal_nonce(key: bytes, nonce: bytes, aad: bytes, pt: bytes) -> bytes:
    r, s = one_time_key(key, nonce)
    ct = xor(pt, keystream(key, nonce, len(pt)))
    return ct + tag_of(accumulate(r, mac_data(aad, ct)), s)


def seal(key: bytes, counter: int, aad: bytes, pt: bytes) -> bytes:
    """Ciphertext | tag under Nebula's nonce for `counter`."""
    return seal_nonce(key, nebula_nonce(counter), aad, pt)


def accumulator(key: bytes, counter: int, aad: bytes, pt: bytes) -> int:
    nonce = nebula_nonce(counter)
    r, _ = one_time_key(key, nonce)
    return accumulate(r, mac_data(aad, xor(pt, keystream(key, nonce, len(pt)))))


# ---- directed targets ------------------------------------------------------------------------

def _zero_tag(r, s):
    """h + s = 2^128 with a carry out of every word: the tag is all zero. Word 0 carries only if
    s's word 0 is not zero; then every word above sums to 2^32 - 1 plus the carry."""
    return (1 << 128) - s if s & 0xFFFFFFFF else None


def _carry_word0(r, s):
    """A carry out of word 0 of h + s and out of no other word: h = 2^32 - s's word 0."""
    s0, s1 = s & 0xFFFFFFFF, (s >> 32) & 0xFFFFFFFF
    return (1 << 32) - s0 if s0 and s1 != 0xFFFFFFFF else None


# name -> the accumulator value, or a function of the one-time key (None: not at this counter)
EDGE_TARGETS = {
    "0": 0, "1": 1, "2": 2, "3": 3, "4": 4, "5": 5,
    "p-1": P - 1, "p-2": P - 2,
    "2^128-1": (1 << 128) - 1, "2^128": 1 << 128, "2^128+1": (1 << 128) + 1,
    "2^104-1": (1 << 104) - 1, "2^26-1": (1 << 26) - 1, "2^52-1": (1 << 52) - 1,
    "tag_zero_carry_every_word": _zero_tag,
    "carry_out_of_word0_only": _carry_word0,
}
SHAPES = ("relay", "data")
KEYS = (bytes(range(0x80, 0xA0)), bytes((7 * i + 3) & 0xFF for i in range(32)))


def target_value(name: str, key: bytes, counter: int):
    t = EDGE_TARGETS[name]
    return t(*one_time_key(key, nebula_nonce(counter))) if callable(t) else t


def _filler(label: str, n: int) -> bytes:
    return hashlib.shake_256(label.encode()).digest(n)


def solve(key: bytes, target, shape: str, label: str = ""):
    """The first counter in 1..MAX_COUNTER, with the packet (counter, aad, plaintext), whose
    accumulator is `target` (an integer in [0, p), or a function (r, s) -> integer or None).
    relay: len = 0 and 3 AAD blocks, the last one solved. data: a 16-byte AAD and 3 payload
    blocks; the last ciphertext block is solved and the plaintext is it XOR its keystream
    (bytes 32..47 of the payload's keystream). None when no counter works."""
    assert shape in SHAPES
    fill = _filler(f"{shape}/{label}/{key.hex()}", 48)
    for counter in range(1, MAX_COUNTER + 1):
        nonce = nebula_nonce(counter)
        r, s = one_time_key(key, nonce)
        t = target(r, s) if callable(target) else target
        if t is None or r == 0:
            continue
        assert 0 <= t < P
        if shape == "relay":
            head = fill[:32]                       # two whole AAD blocks
            lens = struct.pack("<QQ", 48, 0)
        else:
            head = fill[:16] + fill[16:48]         # the AAD block, two ciphertext blocks
            lens = struct.pack("<QQ", 16, 48)
        h_prev = accumulate(r, head)
        rinv = pow(r, P - 2, P)
        blk = ((t * rinv - int.from_bytes(lens, "little") - (1 << 128)) * rinv - h_prev - (1 << 128)) % P
        if blk >> 128:
            continue
        last = blk.to_bytes(16, "little")
        if shape == "relay":
            return counter, head + last, b""
        ct = head[16:] + last
        return counter, head[:16], xor(ct, keystream(key, nonce, 48))
    return None


def all_ff(key: bytes, shape: str, counter: int = 7):
    """Every message limb at its maximum in every round: 40 AAD blocks of 0xFF (relay), or a
    16-byte AAD and a 640-byte payload whose ciphertext is all 0xFF (data)."""
    if shape == "relay":
        return counter, b"\xff" * 640, b""
    return counter, b"\xff" * 16, xor(b"\xff" * 640, keystream(key, nebula_nonce(counter), 640))


def vectors():
    """The 34 directed packets, without sealed bytes: every target in both shapes (the keys
    alternate), then the all-0xFF packet of each shape. Raises if a target is not reached."""
    out = []
    for shape in SHAPES:
        for name, t in EDGE_TARGETS.items():
            key = KEYS[len(out) % 2]
            got = solve(key, t, shape, name)
            if got is None:
                raise ValueError(f"{shape}/{name}: no counter up to {MAX_COUNTER} reaches the target")
            counter, aad, pt = got
            out.append({"shape": shape, "target": name, "key": key.hex(), "counter": counter,
                        "aad": aad.hex(), "plaintext": pt.hex()})
    for shape in SHAPES:
        key = KEYS[len(out) % 2]
        counter, aad, pt = all_ff(key, shape)
        out.append({"shape": shape, "target": "all_ff", "key": key.hex(), "counter": counter,
                    "aad": aad.hex(), "plaintext": pt.hex()})
    return out
