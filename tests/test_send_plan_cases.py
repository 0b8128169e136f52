"""CPU: the TX send plan's directed cases (tests/send_plan_cases.py). Every case reaches its stated
condition, and the sequential model (WriteBatch's packing loop restated), the parallel model (the
device form's decomposition) and the host form (neb_tx_send_plan_host) give the same plan; the
reference tests' own shapes (tests/golden/send_plan_writebatch.json) group as those tests expect."""
import pytest

import send_plan_cases as SC
import send_plan_ref as M

DIRECTED = SC.directed()


def _agree(b):
    detail = {}
    seq, par, host = M.sequential(b), M.parallel(b, detail), SC.host_plan(b)
    assert par == seq
    assert host == seq
    # the plan's own invariants
    n_ok = sum(1 for s in seq.send_status if s == M.OK)
    assert len(seq.iov) == n_ok == sum(e[1] for e in seq.entries)
    for k, e in enumerate(seq.entries):
        assert e[0] == sum(x[1] for x in seq.entries[:k]) and 1 <= e[1] <= max(b.max_segments, 1)
        assert e[1] == 1 or e[4] <= M.MAX_BYTES
        if b.chunk_packets:
            assert e[0] // b.chunk_packets == (e[0] + e[1] - 1) // b.chunk_packets
    return seq, detail


@pytest.mark.parametrize("case", DIRECTED, ids=[c.name for c in DIRECTED])
def test_directed_case(case):
    seq, detail = _agree(case.batch)
    assert case.reaches(seq, detail), (SC.shape(seq), seq.send_status[:16], detail.get("hard", [])[:16])


def test_parity_chain_dropping_the_first_wire_moves_every_boundary():
    """Lengths strictly fall, so every run is two packets and each run's end decides the next one's
    start along the whole batch: without the first wire every boundary moves by one. A wrong
    composition order or a carry lost between two tiles of a scan shows here."""
    full, _ = _agree(SC.parity_chain(False))
    dropped, detail = _agree(SC.parity_chain(True))
    assert SC.shape(full) == [(2, 4200 - 2 * k) for k in range(2048)] + [(1, 0)]
    assert SC.shape(dropped) == [(2, 4199 - 2 * k) for k in range(2048)]
    assert len(detail["plateaus"]) == 4096 and detail["hard"] == [1]
    first_full = {full.iov[e[0]][2] for e in full.entries}
    first_dropped = {dropped.iov[e[0]][2] for e in dropped.entries}
    assert first_full == set(range(0, 4097, 2)) and first_dropped == set(range(1, 4097, 2))
    assert not (first_full & first_dropped)


def test_random_batches():
    hit_absorb = hit_unroutable = hit_chunk = 0
    for b in SC.random_batches(20261021, 3000):
        seq, detail = _agree(b)
        hit_absorb += any(o for o in detail["o"])
        hit_unroutable += M.UNROUTABLE in seq.send_status
        hit_chunk += bool(b.chunk_packets) and len(seq.iov) > b.chunk_packets
    assert hit_absorb > 100 and hit_unroutable > 100 and hit_chunk > 100


@pytest.mark.parametrize("g", SC.golden(), ids=[g[0] for g in SC.golden()])
def test_reference_test_shapes(g):
    name, b, cs, names = g
    seq, _ = _agree(b)
    assert [(e[1], e[2], names[e[3]]) for e in seq.entries] == [(e["niov"], e["seg_size"], e["dst"]) for e in cs["entries"]]
    assert [i for i, s in enumerate(seq.send_status) if s == M.UNROUTABLE] == cs["unroutable"]
    assert sum(e[1] for e in seq.entries) == len(cs["sizes"]) - len(cs["unroutable"])
