"""Directed replay-window cases for the device receive's parallel form (nebula_amd/csrc/rxwin.hip),
shared by tests/test_rxwin_cases.py (CPU: what the cases reach, and the model against the oracle on
them) and tests/test_gpu_rxwin_edges.py (GPU: every case through every form of the receive).

A case is a window length, a history per window (counters fed through Update before the first
batch), and one or more batches of (tunnel, counter, forged) arrivals, each batch strict (the device
form only, NEB_KNOB_RX_STRICT) or not. Tunnels are numbered in the order of their window slots, so
the run order the sort must produce is the stable sort of a batch by tunnel, tunnels without a
window last (rx_keys_kernel, rx_sort_pass_kernel). No engine, no AEAD: pure Python over
oracle/replay_oracle.py (tools/ is put on the path for the tests' import of rxwin_model).

Families:
  arith     scripted steps relative to the running maximum, per length and start state
  position  run heads, run lengths and carried maxima placed in the 256-position scan blocks
  carried   state left from one batch to the next on one window set
  forged    the two above with a forgery in a role at an edge (non-strict)
"""
from __future__ import annotations

import os
import random
import re
import sys
from functools import lru_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in ("oracle", "tools"):
    if os.path.join(ROOT, _p) not in sys.path:
        sys.path.insert(0, os.path.join(ROOT, _p))
import replay_oracle as R  # noqa: E402

LENGTHS = (1, 2, 16, 32, 64, 128, 1024, 65536)
P32 = 1 << 32


@lru_cache(maxsize=None)
def constants():
    """The kernels' geometry, read from the sources (never restated here)."""
    csrc = os.path.join(ROOT, "nebula_amd", "csrc")
    hpp = open(os.path.join(csrc, "rxwin.hpp")).read()
    hip = open(os.path.join(csrc, "rxwin.hip")).read()

    def num(pat, text=hpp):
        return int(re.search(pat, text).group(1))

    assert re.search(r"kRxBlock = kRxThreads \* kRxItems", hpp)
    sort_threads = num(r"so\.per_blk = (\d+)u \* so\.items", hip)
    return dict(block=num(r"kRxThreads = (\d+)") * num(r"kRxItems = (\d+)"),
                sort_blocks=num(r"kRxSortBlocks = (\d+)"), sort_digit=num(r"kRxSortDigit = (\d+)"),
                sort_threads=sort_threads, risky=1 << num(r"kRxRiskyCounter = 1ull << (\d+)"))


class Case:
    def __init__(self, name, family, length, history, batches, kinds=None, labels=None, absent=()):
        self.name, self.family, self.length = name, family, length
        self.history = history            # tunnel -> [counters fed through Update]
        self.batches = batches            # [(arrivals [(tunnel, counter, forged)], strict)]
        self.kinds = kinds                # per arrival of batch 0: the script step that made it
        self.labels = labels or {}        # tunnel -> (start state, script)
        self.absent = frozenset(absent)   # tunnels with no window
        self._replay = None
        self.ntun = 1 + max(max(t for b, _ in batches for t, _, _ in b), max(history, default=0))

    @property
    def strict(self):
        return all(s for _, s in self.batches)

    @property
    def arrivals(self):
        return [a for b, _ in self.batches for a in b]

    def replayed(self):
        if self._replay is None:
            self._replay = replay(self)
        return self._replay

    def __repr__(self):
        return f"Case({self.name})"


def run_order(arrivals, absent=()):
    """Arrival indices in run order: stable by window slot, no window last."""
    return sorted(range(len(arrivals)), key=lambda i: (arrivals[i][0] in absent, 0 if arrivals[i][0] in absent
                                                       else arrivals[i][0]))


def replay(case):
    """The sequential receive over the case. Returns (statuses, decrypted flags, final windows,
    records): one record per (batch, window touched) with the window before and after."""
    wins = {}
    for t in range(case.ntun):
        if t in case.absent:
            continue
        w = R.Bits(case.length)
        for c in case.history.get(t, []):
            w.update(c)
        wins[t] = w
    status, dec, records = [], [], []
    for bi, (arr, strict) in enumerate(case.batches):
        before = {t: (w.current, list(w.bits), w.lost) for t, w in wins.items() if any(a[0] == t for a in arr)}
        verdicts = [R.BAD_KEY if t in case.absent else (R.AUTH_FAILED if f else R.OK) for t, _, f in arr]
        st, d = R.rx_sequential(wins, [a[0] for a in arr], [a[1] for a in arr], verdicts)
        for t, (cur0, bits0, lost0) in before.items():
            w = wins[t]
            idx = [i for i, a in enumerate(arr) if a[0] == t]
            records.append(dict(case=case.name, batch=bi, tunnel=t, label=case.labels.get(t), length=case.length,
                                cur0=cur0, bits0=bits0, lost0=lost0, cur=w.current, bits=list(w.bits), lost=w.lost,
                                run=[arr[i][1] for i in idx], forged=any(arr[i][2] for i in idx),
                                status=[st[i] for i in idx], strict=strict))
        status += st
        dec += d
    return status, dec, wins, records


# ---- (a) arithmetic -----------------------------------------------------------------------------

def starts(length):
    """Start states: name -> current before the batch."""
    n62 = (1 << 62) - 4 * length - 40
    return {"zero": 0, "lenm1": length - 1, "len": length, "steady": 5 * length + 3, "w62": 7 * length + 61,
            "p32m3": P32 - 3, "p32p7": P32 + 7, "n62a": n62, "n62b": n62}


def history_for(cur, length):
    """Counters that leave `current` = cur with the two oldest counters of the window received,
    holes at cur - 1 and cur - 2 and most of the window empty."""
    if cur == 0:
        return []
    return sorted(c for c in {cur - length + 1, cur - length + 2, cur - length // 2, cur - 3, cur} if 1 <= c <= cur)


SCRIPTS = ("full", "small", "adv_lm1", "adv_l", "adv_lp1")


def script(name, start, cur0, length, forge=()):
    """[(counter, kind, forged)]: steps relative to the running maximum m of the genuine counters."""
    L, m, out = length, cur0, []

    def emit(c, kind):
        nonlocal m
        if c < 0:
            return
        forged = kind in forge
        out.append((c, kind, forged))
        if not forged:
            m = max(m, c)

    def probes():
        emit(m - L, "-len")       # just out
        emit(m - L + 1, "-len+1")  # the oldest counter still in
        emit(m, "0")

    def advance(total):
        if total <= 0:
            emit(m, "0")
        elif total == 1:
            emit(m + 1, "+1")
        else:
            emit(m + 1, "+1")
            emit(m + total - 1, "jump")

    if name == "full":
        emit(m + 1, "+1")
        emit(m, "0")
        emit(0, "zero")
        emit(m + 3, "+3")
        emit(m - 1, "backfill")
        emit(m - 1, "backfill_again")
        emit(m - 2, "backfill")
        jumps = (("+len-1", L - 1), ("+len", L), ("+len+1", L + 1), ("+3len", 3 * L))
        if start == "n62a":  # the counters stay below 2^62: no room for all four
            jumps = jumps[:3]
        elif start == "n62b":
            jumps = (jumps[0], jumps[3])
        for kind, d in jumps:
            a = m + 1
            emit(a, "+1")            # admitted, then pushed out by the jump
            x = m - L
            emit(x, "-len")          # refused: out of the window
            emit(m + d, kind)
            if kind in forge:        # the genuine twin of a forged jump
                emit(m + d, kind + "_twin")
            emit(a, "left_again")
            emit(x, "refused_again")  # its earlier refusal still holds
            probes()
        emit(0, "zero")
    elif name == "small":
        emit(m + 5, "+5")
        emit(m - 2, "backfill")
        emit(m - 2, "backfill_again")
        probes()
    else:
        advance({"adv_lm1": L - 1, "adv_l": L, "adv_lp1": L + 1}[name])
        probes()
        emit(m - 1, "backfill")
    return out


def _interleave(runs):
    """Round-robin over the runs, each run's order kept: [(tunnel, item)]."""
    out, k = [], 0
    while any(k < len(r) for r in runs):
        out += [(t, r[k]) for t, r in enumerate(runs) if k < len(r)]
        k += 1
    return out


# at length 65536 a window costs 65536 bitmap reads to compare: the runs that carry a condition
_BIG_RUNS = {("zero", "full"), ("lenm1", "full"), ("p32m3", "full"), ("n62a", "full"), ("n62b", "full"),
             ("p32m3", "small"), ("w62", "small"), ("steady", "small"), ("steady", "adv_lm1"), ("len", "adv_lm1"),
             ("p32p7", "adv_l"), ("steady", "adv_lp1")}


def arith_runs(length):
    return [(s, sc) for s in starts(length) for sc in SCRIPTS if length < 65536 or (s, sc) in _BIG_RUNS]


def arith_case(length, runs=None, forge=(), name=None):
    runs = arith_runs(length) if runs is None else runs
    st = starts(length)
    history, labels, seqs = {}, {}, []
    for t, (s, sc) in enumerate(runs):
        history[t] = history_for(st[s], length)
        labels[t] = (s, sc)
        seqs.append(script(sc, s, st[s], length, forge))
    mixed = _interleave(seqs)
    arr = [(t, c, f) for t, (c, _, f) in mixed]
    kinds = [k for _, (_, k, _) in mixed]
    return Case(name or f"arith_{length}", "forged" if forge else "arith", length, history, [(arr, not forge)], kinds,
                labels)


def arith_one(length):
    """One window (a key_hint batch, and the sort's identity path): the full script across 2^32."""
    return arith_case(length, [("p32m3", "full")], name=f"arith1_{length}")


# ---- (b) positions ------------------------------------------------------------------------------

def _spread(runs):
    """Arrival order: every run spread over the whole batch in proportion, its own order kept."""
    keyed = [((j + 0.5) / len(r), t, j) for t, r in enumerate(runs) for j in range(len(r))]
    return [(t, runs[t][j], False) for _, t, j in sorted(keyed)]


def _traffic(seed, cur0, n):
    """Ordinary traffic: mostly +1, some small jumps, backfills and duplicates."""
    rng, cur, out = random.Random(seed), cur0, []
    for _ in range(n):
        r = rng.random()
        if r < 0.7:
            cur += 1
            out.append(cur)
        elif r < 0.8:
            cur += rng.randrange(2, 6)
            out.append(cur)
        else:
            out.append(max(1, cur - rng.randrange(0, 9)))
    return out


P1_SIZES = (1, 255, 256, 257, 100, 154, 1 + 4 * 256 + 10)


def position_heads(length):
    """Seven windows whose runs are 1, 255, 256, 257, 100, 154 and 1035 long: heads at block offsets
    0 (positions 256 and 512), 1 (positions 1 and 769) and 255 (position 1023); the 257-run's last
    packet is a block's first; the last run's maximum is its head, in block 3, and its blocks 4..8
    hold only smaller counters, the last block partial. Its counters repeat after length/2 + 40
    packets (an equal pair lies more than two blocks apart), then probe the window's lower edge."""
    L = length
    history = {t: [1, 2, 3] for t in range(6)}
    runs = [_traffic(10 + t, 3, n) for t, n in enumerate(P1_SIZES[:6])]
    cur0 = 5 * L + 3
    history[6] = history_for(cur0, L)
    H, mod = cur0 + L // 2, L // 2 + 40
    last = [H]
    for j in range(1, P1_SIZES[6]):
        last.append(H - 1 - (j * 5) % mod if j < 700 else H - L - 20 + j % 40)
    runs.append(last)
    return Case(f"pos_heads_{L}", "position", L, history, [(_spread(runs), True)])


def position_carry():
    """Length 1024. Window 1's run (head at position 10) reaches 2^32 - 1 at the end of block 0, has
    2^32 in block 1 among smaller counters, and probes 2^32 - 1024 (out only if the carried maximum
    is 2^32) from block 2 on. Window 2 crosses a block with both words of its maximum non-zero.
    Window 3 (head at position 1280) leaves 3 * 2^32 + 5 in block 5; block 6's own maximum is
    2 * 2^32 + 0xFFFFFFxx (lower, with the larger low word); block 7 probes the lower edge."""
    L = 1024
    history, runs = {0: [1, 2, 3]}, [_traffic(3, 3, 10)]
    c1 = P32 - 1 - 246
    history[1] = history_for(c1, L)
    r1 = [c1 + 1 + j for j in range(246)]
    r1 += [P32] + [c1 - 1 - j % 300 for j in range(255)]
    r1 += [P32 - L - 8 + j % 16 for j in range(256 + 5)]
    runs.append(r1)
    c2 = 3 * P32 + 0x00F00000
    history[2] = history_for(c2, L)
    runs.append(_traffic(5, c2, 507))
    top = 3 * P32 + 5
    c3 = top - 256
    history[3] = history_for(c3, L)
    r3 = [c3 + 1 + j for j in range(256)]
    r3 += [2 * P32 + 0xFFFFFF00 + j % 250 for j in range(256)]
    r3 += [top - L - 8 + j % 16 for j in range(100)]
    runs.append(r3)
    return Case("pos_carry", "position", L, history, [(_spread(runs), True)])


BIG_N = 3 + 66 * 256 + 10


def position_lookback():
    """Length 1024, 16909 packets: a 3-packet run of the lower slot, then one window's run of
    66 * 256 + 10. Its maximum M is in block 0; blocks 1..64 stay within [M - 1012, M - 513]; the
    last blocks probe M - 1024, which is out only when block 0's maximum is carried past the first
    64 blocks of the lookback."""
    L = 1024
    cur0 = 5 * L + 3
    history = {0: [1, 2, 3], 1: history_for(cur0, L)}
    M_ = cur0 + 20000
    n1 = BIG_N - 3
    r1 = [cur0 + 1 + j for j in range(5)] + [M_]
    for j in range(6, n1):
        r1.append(M_ - 513 - (j * 7) % 500 if j < 65 * 256 - 3 else M_ - L - 8 + j % 16)
    arr = [(1, c, False) for c in r1]
    for pos, c in ((5000, 4), (9000, 5), (BIG_N - 1, 5)):
        arr.insert(pos, (0, c, False))
    return Case("pos_lookback", "position", L, history, [(arr, True)])


# ---- (c) carried state --------------------------------------------------------------------------

def carried_twice():
    L = 1024
    history = {t: history_for(5 * L + 3, L) for t in range(3)}
    runs = [_traffic(20 + t, 5 * L + 3, 70) + [5 * L + 3 - L, 0, 7 * L] for t in range(3)]
    b = _spread(runs)
    return Case("carried_twice", "carried", L, history, [(b, True), (list(b), True)])


def carried_small_after_large():
    L = 64
    history = {t: [1, 2, 3] for t in range(3)}
    runs = [_traffic(30 + t, 3, 200) for t in range(3)]
    big = _spread(runs)
    # the small batch: each window's last counters again (same keys at other arrival indices), then new ones
    small = []
    for t in range(3):
        top = max(runs[t])
        small += [(t, c, False) for c in runs[t][-5:] + [top + 1, top + 1, top + 70]]
    return Case("carried_small_after_large", "carried", L, history, [(big, True), (small, True)])


def carried_host_then_strict():
    """A forgery sends window 0 to the host in a non-strict batch (its settle has written scratch bits
    by then); the strict batch after it uses the same bitmap words of window 0."""
    L = 128
    cur0 = 5 * L + 3
    history = {0: history_for(cur0, L), 1: history_for(cur0, L)}
    a = [(0, cur0 + 1, False), (0, cur0 + 2, False), (0, cur0 + 4, True), (0, cur0 + 5, False), (0, cur0 - 1, False)]
    b = [(1, c, False) for c in _traffic(41, cur0, 20)]
    first = [x for pair in zip(a, b) for x in pair] + b[len(a):]
    second = [(0, cur0 + 3, False), (0, cur0 + 4, False), (0, cur0 + 6, False), (0, cur0 - 2, False),
              (0, cur0 + 5, False), (1, cur0 + 40, False), (0, cur0 + 7, False)]
    return Case("carried_host_then_strict", "carried", L, history, [(first, False), (second, True)])


# ---- (d) forged variants ------------------------------------------------------------------------

def forged_jump(length):
    """The full script with the jump of exactly len forged (the window must not move), then genuine."""
    return arith_case(length, [(s, "full") for s in ("zero", "steady", "p32m3")], forge=("+len",),
                      name=f"forged_jump_{length}")


def forged_twin():
    """A forged first occurrence at run position 255, its genuine twin at 256 (the next scan block);
    and a tunnel with no window, whose packets sort last and come back BAD_KEY untouched."""
    L = 1024
    history = {0: [1, 2, 3], 1: [1, 2, 3]}
    r0 = _traffic(50, 3, 200)
    r1 = _traffic(51, 3, 300)
    x = max(r1[:55]) + 2
    r1[55] = r1[56] = x
    runs = [r0, r1, [3 + j for j in range(20)]]
    arr = _spread(runs)
    seen = False
    for i, (t, c, _) in enumerate(arr):  # the first arrival of x is the forgery
        if t == 1 and c == x and not seen:
            arr[i] = (t, c, True)
            seen = True
    return Case("forged_twin", "forged", L, history, [(arr, False)], absent={2})


@lru_cache(maxsize=None)
def cases():
    out = [arith_case(L) for L in LENGTHS] + [arith_one(L) for L in LENGTHS]
    out += [position_heads(1024), position_heads(64), position_carry(), position_lookback()]
    out += [carried_twice(), carried_small_after_large(), carried_host_then_strict()]
    out += [forged_jump(L) for L in (2, 64, 1024)] + [forged_twin()]
    return {c.name: c for c in out}


# ---- conditions ---------------------------------------------------------------------------------

def step_conditions(case_list, lengths=LENGTHS):
    """Unmet (length, kind, outcome): every step kind reached with the oracle's outcome."""
    got = set()
    for c in case_list:
        st = c.replayed()[0]
        got |= {(c.length, k, s) for k, s in zip(c.kinds, st)}
    want = []
    for L in lengths:
        ok = [("+1", R.OK), ("+3", R.OK), ("+len", R.OK), ("+len+1", R.OK), ("+3len", R.OK)]
        no = [("0", R.REPLAY), ("zero", R.REPLAY), ("-len", R.REPLAY), ("backfill_again", R.REPLAY),
              ("left_again", R.REPLAY), ("refused_again", R.REPLAY)]
        # at length 1 a step of len - 1 is the current counter again, the oldest counter in is current
        # and there is no hole to fill
        ok += [("+len-1", R.OK), ("-len+1", R.OK), ("backfill", R.OK)] if L >= 2 else []
        no += [("-len+1", R.REPLAY)] if L >= 2 else [("+len-1", R.REPLAY), ("-len+1", R.REPLAY)]
        want += [(L, k, s) for k, s in ok + no]
    return [w for w in want if w not in got]


def _ring_props(start, count, L):
    """(wraps, straddles a word boundary) of the circular slot range the kernel masks with
    rx_ring_mask: count < len (a whole ring takes another branch), except that at length 2 the only
    range over slot 1 -> 0 is the whole ring."""
    if count <= 0 or (count >= L and L != 2):
        return False, False
    wraps = start + count > L and start > 0
    straddles = any((start + k) % L % 64 == 63 and (start + k + 1) % L != 0 for k in range(min(count, L) - 1))
    return wraps, straddles


def window_facts(rec):
    """What one window's batch reaches, from the oracle's window before and after it."""
    L, mask, cur0, cur = rec["length"], rec["length"] - 1, rec["cur0"], rec["cur"]
    lo = cur0 - L + 1 if cur0 >= L else 1
    hi = cur - L if cur >= L else 0
    base = cur - L if (cur >= L and cur - L > cur0) else cur0
    ehi = min(hi, cur0)
    facts = set()
    cw, cs = _ring_props((base + 1) & mask, cur - base, L)
    lw, ls = _ring_props(lo & mask, ehi - lo + 1, L) if ehi >= lo else (False, False)
    facts |= {n for n, v in (("clear_wraps", cw), ("clear_straddles", cs), ("leave_wraps", lw),
                             ("leave_straddles", ls)) if v}
    if cur - base == L:
        facts.add("clear_len")
    if cur - base == L - 1:
        facts.add("clear_len-1")
    adm_left = sum(1 for c, s in zip(rec["run"], rec["status"]) if s == R.OK and lo <= c <= hi)
    old_left = sum(1 for e in range(lo, ehi + 1) if rec["bits0"][e & mask])  # (at most len counters)
    if adm_left and old_left:
        facts.add("both_left")
    if cur0 < L <= cur:
        facts.add("warmup_crossed")
    return facts


def window_conditions(records, lengths=LENGTHS):
    """Unmet (length, fact) over the arithmetic windows."""
    got = set()
    for r in records:
        got |= {(r["length"], f) for f in window_facts(r)}
    want = []
    for L in lengths:
        if L < 2:
            continue
        names = ["clear_wraps", "leave_wraps", "clear_len", "clear_len-1", "both_left", "warmup_crossed"]
        if L >= 128:
            names += ["clear_straddles", "leave_straddles"]
        want += [(L, n) for n in names]
    return [w for w in want if w not in got]


def layout(case, batch=0):
    """The predicted run order of a batch and what the scan blocks publish: dict with n, order,
    tun / ctr (run order), heads, run lengths, items, per_blk and pub[b] = (tunnel, segmented max at
    block b's last position, whether a later block of the same run reads it)."""
    k = constants()
    arr = case.batches[batch][0]
    n = len(arr)
    order = run_order(arr, case.absent)
    tun = [arr[i][0] for i in order]
    ctr = [arr[i][1] for i in order]
    heads = [p for p in range(n) if p == 0 or tun[p] != tun[p - 1]]
    lens = [b - a for a, b in zip(heads, heads[1:] + [n])]
    B = k["block"]
    pub = []
    for b in range((n + B - 1) // B):
        e = min(n, (b + 1) * B) - 1
        s = max(max(h for h in heads if h <= e), b * B)
        pub.append((tun[e], max(ctr[s:e + 1]), e + 1 < n and tun[e + 1] == tun[e]))
    items = -(-n // (k["sort_threads"] * k["sort_blocks"]))
    return dict(n=n, order=order, tun=tun, ctr=ctr, heads=heads, lens=lens, pub=pub, items=items,
                per_blk=k["sort_threads"] * items, block=B)


def position_facts(case):
    lay = layout(case)
    B, n, tun, ctr, heads = lay["block"], lay["n"], lay["tun"], lay["ctr"], lay["heads"]
    facts = {f"head_at_{h % B}" for h in heads if h > 0}
    facts |= {f"run_of_{x}" for x in lay["lens"]}
    if n % B:
        facts.add("partial_final_block")
    cur0 = {r["tunnel"]: r["cur0"] for r in case.replayed()[3] if r["batch"] == 0}
    head_of = {}
    for h in heads:
        head_of[tun[h]] = h
    headless = [not any(b * B <= h < (b + 1) * B for h in heads) for b in range(len(lay["pub"]))]
    for b in range(1, len(lay["pub"])):
        p0 = b * B
        h = head_of[tun[p0]]
        if h >= p0:
            continue  # the block starts with a head: nothing carried in
        pre = max(ctr[h:p0])
        if pre <= cur0.get(tun[p0], 0):
            continue
        at = ctr.index(pre, h) // B
        if at == b - 1:
            facts.add("max_in_previous_block")
        if at <= b - 4 and all(headless[q] and lay["pub"][q][1] < pre for q in range(b - 3, b)):
            facts.add("max_three_headless_blocks_back")
        if b - h // B > 64:
            facts.add("head_more_than_64_blocks_back")
    pub = lay["pub"]
    for (t0, v0, r0), (t1, v1, r1) in zip(pub, pub[1:]):
        if t0 == t1 and r0 and r1:
            if v0 == P32 - 1 and v1 == P32:
                facts.add("carry_2^32-1_then_2^32")
            if v1 >> 32 < v0 >> 32 and v1 & (P32 - 1) > v0 & (P32 - 1):
                facts.add("carry_halves_disagree")
    if any(r and v >> 32 and v & (P32 - 1) for _, v, r in pub):
        facts.add("carry_both_words")
    # equal counters, the first admitted and the second refused, in other scan and sort blocks
    st = case.replayed()[0]
    arr = case.batches[0][0]
    pos = {i: p for p, i in enumerate(lay["order"])}
    first = {}
    for i, (t, c, _) in enumerate(arr):
        j = first.setdefault((t, c), i)
        if j != i and st[j] == R.OK and st[i] == R.REPLAY and pos[i] // B != pos[j] // B and \
                i // lay["per_blk"] != j // lay["per_blk"]:
            facts.add("equal_counters_across_blocks")
    if lay["items"] == 2 and len(set(tun)) > 1:
        facts.add("two_items_sorted")
    return facts


POSITION_WANT = {
    "pos_heads": {"head_at_0", "head_at_1", "head_at_255", "run_of_1", "run_of_255", "run_of_256", "run_of_257",
                  "max_in_previous_block", "max_three_headless_blocks_back", "partial_final_block",
                  "equal_counters_across_blocks"},
    "pos_carry": {"carry_2^32-1_then_2^32", "carry_both_words", "carry_halves_disagree", "partial_final_block"},
    "pos_lookback": {"head_more_than_64_blocks_back", "two_items_sorted", "partial_final_block"},
}


def position_conditions(case_list):
    """Unmet (kind of case, fact); every kind of POSITION_WANT must be there."""
    missing = []
    for kind, want in POSITION_WANT.items():
        mine = [c for c in case_list if c.name.startswith(kind)]
        if not mine:
            missing += [(kind, f) for f in sorted(want)]
        for c in mine:
            missing += [(c.name, f) for f in sorted(want - position_facts(c))]
    return missing


def strict_violations(case):
    """Why a strict batch could not stay on the device: a forgery, a tunnel without a window, a
    counter or a current at or above the risky bound."""
    risky = constants()["risky"]
    bad = []
    for r in case.replayed()[3]:
        if r["strict"] and (r["forged"] or max([r["cur0"], r["cur"]] + r["run"]) >= risky):
            bad.append((case.name, r["batch"], r["tunnel"]))
    for bi, (arr, strict) in enumerate(case.batches):
        if strict and any(t in case.absent or f for t, _, f in arr):
            bad.append((case.name, bi, "absent or forged"))
    return bad
