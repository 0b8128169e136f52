"""What the connection table (neb_conntrack_*) costs on a device-resident batch, beside the read-back
it replaces.

Workload: --n firewall packets (default 64 Ki) of TCP/IPv4 flows, drawn evenly from the table's flows.
Table states: 1 flow, 4096 flows and 1 Mi flows, each table at half load (capacity = 2 x flows).
Measures, per state:

  a_lookup_hits      neb_conntrack_lookup_batch alone, every packet an established flow (device events
                     around a run of launches: the lookup kernel, the scan and the scatter), and
  a_lookup_1pct_miss the same with 1 % of the packets from flows the table does not hold, with the hold
                     marks and the work list written
  c_host_form        neb_conntrack_lookup_batch_host's C entry point on one thread over a host-only
                     table of the same flows (wall time of the calling thread)
  d_through_host     what the call replaces around the caller's own map: d_fw (48 bytes per packet)
                     copied to pinned host memory, one flag per packet uploaded; the host's lookups
                     themselves are c_host_form's (wall time)
  add_new            neb_conntrack_add_batch of --n flows the table does not hold (both launches), each
                     timed run on a table refilled outside the window
  compact            neb_conntrack_compact of the table (wall time: it blocks)

  b_pipeline_plain     neb_rx_open_wire_batch -> neb_rx_plain_from_wire -> neb_rx_coalesce_batch,
  b_pipeline_inner     the same with neb_rx_inner_batch in the middle, and
  b_pipeline_conntrack the same with the lookup, holding, between the inner resolve and the coalescer:
                       tools/rx_inner_bench.py's workload (--n wire packets of 1364 bytes, one TCP flow
                       per tunnel; 1 tunnel and 4096 tunnels), every flow tracked, in tables of 1, 4096
                       and 1 Mi flows at half load; the three alternate step by step, the packets are
                       re-sealed on the device outside the timed window, and all three come from one
                       run, so the lookup's cost in its place stands beside the inner resolve's own

Every figure is the median over windows of at least --window seconds of timed work. Before timing the
device form must equal the host form.

  python tools/conntrack_bench.py --out profiles/conntrack/bench.jsonl
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nebula_amd import _lib as L  # noqa: E402
from nebula_amd import firewall as F  # noqa: E402
from nebula_amd import outside as O  # noqa: E402
from nebula_amd.connection_state import rx_open_wire_batch_device  # noqa: E402
from nebula_amd.noiseutil import Engine  # noqa: E402

T0 = 10**12


def flows(first, count):
    """`count` TCP/IPv4 flows numbered from `first`: 10.a.b.c:port -> 10.200.0.1:443."""
    i = np.arange(first, first + count, dtype=np.uint32)
    fw = np.zeros(count, L.FW_PACKET_DTYPE)
    fw["family"], fw["protocol"], fw["local_port"], fw["gateway"] = 4, 6, 443, L.GATEWAY_NONE
    fw["local_addr"][:, :4] = (10, 200, 0, 1)
    fw["remote_addr"][:, 0] = 10
    fw["remote_addr"][:, 1] = (i >> 16) & 255
    fw["remote_addr"][:, 2] = (i >> 8) & 255
    fw["remote_addr"][:, 3] = i & 255
    fw["remote_port"] = 1024 + (i >> 24)
    return fw


def pipelines(eng, a, emit, torch):
    """Measure b: the receive chain with and without the lookup, over rx_inner_bench's workload."""
    import rx_inner_bench as RI  # (tools/ is this script's directory)

    n = a.n
    for ntun, nflows in ((1, 1), (4096, 4096), (4096, 1 << 20)):
        case = RI.Case(eng, L.ALG_AESGCM, n, ntun, False)
        try:
            nwrites = case.check()  # ends with the inner resolve's d_fw of every packet
            batch = max(n, 1 << 16)
            with F.Conntrack(eng, 2 * nflows, seed=7, max_batch=batch) as ct:
                d_inc = torch.zeros(batch, dtype=torch.uint8, device=case.dev)
                d_res = torch.zeros(batch * 8, dtype=torch.uint8, device=case.dev)
                ct.add_device(case.d_fw, d_inc, n, T0, d_res)  # the batch's own flows, one per tunnel
                for at in range(0, nflows - ntun, 1 << 16):  # and the other flows of the table
                    part = flows(at, min(1 << 16, nflows - ntun - at))
                    ct.add_device(case.up(part), d_inc, len(part), T0, d_res)
                assert ct.count()[0] == nflows
                d_v = torch.zeros(n, dtype=torch.uint8, device=case.dev)
                d_c = torch.zeros(4, dtype=torch.int32, device=case.dev)
                d_work = torch.zeros(n * L.CT_WORK_DTYPE.itemsize, dtype=torch.uint8, device=case.dev)

                def with_lookup():
                    rx_open_wire_batch_device(case.eng, case.alg, case.dw, case.d_pk, case.arena, case.d_status, case.hint)
                    O.inner_device(case.eng, case.peers, case.d_pk, case.d_status, case.d_epoch, case.arena, case.d_plain, case.d_fw,
                                   case.d_inner)
                    ct.lookup_device(case.d_fw, case.d_inner, n, T0 + 1, d_v, d_c, d_plain=case.d_plain, d_work=d_work, work_cap=n)
                    O.coalesce_batch_device(case.eng, case.d_plain, case.arena, case.d_out, case.d_writes, case.d_nw, case.d_pw,
                                            case.d_ps)
                case.prepare()
                with_lookup()
                torch.cuda.synchronize()
                assert d_c.cpu().numpy().tolist() == [n, 0, 0, 0] and int(case.d_nw.item()) == nwrites, "not every flow is tracked"
                forms = {"b_pipeline_plain": lambda: case.pipeline(False), "b_pipeline_inner": lambda: case.pipeline(True),
                         "b_pipeline_conntrack": with_lookup}
                done, acc, warm = {f: [] for f in forms}, {f: [0.0, 0] for f in forms}, 3
                while any(len(v) < a.windows for v in done.values()):  # alternating, step by step
                    for f, fn in forms.items():
                        case.prepare()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        fn()
                        e1.record()
                        e1.synchronize()
                        if warm > 0:
                            continue
                        acc[f][0] += e0.elapsed_time(e1)
                        acc[f][1] += 1
                        if acc[f][0] >= a.window * 1e3:
                            done[f].append(acc[f][0] * 1e3 / acc[f][1])
                            acc[f] = [0.0, 0]
                    warm -= 1
                for f, v in done.items():
                    emit(nflows, f, v[:a.windows], tunnels=ntun, wire_bytes=RI.WIRE, tun_writes=nwrites)
        finally:
            case.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--flows", default="1,4096,1048576")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed work per window, at least")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--measures", default="a,b", help="a: the calls alone (with c, d, add, compact); b: the receive chain")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("conntrack_bench: no GPU (this tool measures on the device only)")
    dev = torch.device("cuda", 0)
    lines = []
    n = a.n
    vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)  # noqa: E731

    def emit(nflows, measure, windows_us, **more):
        lines.append({"tool": "conntrack_bench", "measure": measure, "packets": n, "flows": nflows, "capacity": 2 * nflows,
                      "median_us": round(statistics.median(windows_us), 2), "windows_us": [round(x, 2) for x in windows_us],
                      "window_s": a.window, "device": torch.cuda.get_device_name(0), "build": L.lib().neb_build_id().decode(),
                      **more})
        print(json.dumps(lines[-1]), flush=True)

    def timed_launches(fn):
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        count = 100
        while True:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(count):
                fn()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            if ms >= a.window * 1e3:
                return ms * 1e3 / count
            count = int(count * max(2.0, 1.2 * a.window * 1e3 / max(ms, 1e-3)))

    def wall(fn):
        t0, calls = time.perf_counter(), 0
        while time.perf_counter() - t0 < a.window:
            fn()
            calls += 1
        return (time.perf_counter() - t0) * 1e6 / calls

    rng = np.random.default_rng(1)
    with Engine(0, 4096 + 64) as eng:
        if "b" in a.measures.split(","):
            pipelines(eng, a, emit, torch)
        for nflows in (int(x) for x in a.flows.split(",") if "a" in a.measures.split(",")):
            table = flows(0, nflows)
            hits = table[rng.integers(0, nflows, n)]
            mixed = hits.copy()
            miss_at = rng.choice(n, n // 100, replace=False)
            mixed[miss_at] = flows(1 << 25, len(miss_at))
            fresh = flows(1 << 26, n)
            batch = 1 << 16
            with F.Conntrack(eng, 2 * nflows, seed=7, max_batch=max(n, batch)) as ct, \
                    F.Conntrack(None, 2 * nflows, seed=7, max_batch=max(n, batch)) as host:
                d_res = torch.zeros(max(n, batch) * 8, dtype=torch.uint8, device=dev)
                d_inc = torch.zeros(max(n, batch), dtype=torch.uint8, device=dev)
                for at in range(0, nflows, batch):
                    part = table[at:at + batch]
                    ct.add_device(up(part), d_inc, len(part), T0, d_res)
                    host.add_host(part, np.zeros(len(part), np.uint8), T0)
                assert ct.count()[0] == nflows == host.count()[0]
                d_hits, d_mixed, d_fresh = up(hits), up(mixed), up(fresh)
                d_st = torch.zeros(n, dtype=torch.int32, device=dev)
                d_v = torch.zeros(n, dtype=torch.uint8, device=dev)
                d_c = torch.zeros(4, dtype=torch.int32, device=dev)
                d_plain = torch.zeros(n * L.PLAIN_PACKET_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                d_work = torch.zeros(n * L.CT_WORK_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                # the device form equals the host form
                ct.lookup_device(d_mixed, d_st, n, T0 + 1, d_v, d_c, d_plain=d_plain, d_work=d_work, work_cap=n)
                torch.cuda.synchronize()
                hv, hwork, hc = host.lookup_host(mixed, np.zeros(n, np.int32), T0 + 1)
                assert d_v.cpu().numpy().tobytes() == hv.tobytes() and d_c.cpu().numpy().tolist() == hc.tolist()
                assert d_work.cpu().numpy().view(L.CT_WORK_DTYPE)[:len(hwork)].tobytes() == hwork.tobytes()
                assert hc.tolist() == [n - len(miss_at), len(miss_at), 0, len(miss_at)]

                def look_hits():
                    ct.lookup_device(d_hits, d_st, n, T0 + 2, d_v, d_c, d_plain=d_plain, d_work=d_work, work_cap=n)

                def look_mixed():
                    d_st.zero_()  # the held packets' statuses, for the next run
                    ct.lookup_device(d_mixed, d_st, n, T0 + 2, d_v, d_c, d_plain=d_plain, d_work=d_work, work_cap=n)

                res = {"a_lookup_hits": [], "a_lookup_1pct_miss": []}
                for _ in range(a.windows):
                    res["a_lookup_hits"].append(timed_launches(look_hits))
                    res["a_lookup_1pct_miss"].append(timed_launches(look_mixed))
                for k, v in res.items():
                    emit(nflows, k, v, launches="lookup kernel, scan, scatter" + ("; and the memset of the statuses" if "miss" in k else ""))

                o_v, o_c, o_st = np.zeros(n, np.uint8), np.zeros(4, np.uint32), np.zeros(n, np.int32)

                def host_form():
                    L.check(L.lib().neb_conntrack_lookup_batch_host(host.handle, vp(hits), vp(o_st), n, T0 + 2, vp(o_v), None, None, None,
                                                                    0, vp(o_c)), "neb_conntrack_lookup_batch_host")
                emit(nflows, "c_host_form", [wall(host_form) for _ in range(a.windows)],
                     clock="wall time of the calling thread on the GPU box's host, outputs allocated once")
                assert o_c.tolist() == [n, 0, 0, 0]

                h_fw = torch.empty(n * L.FW_PACKET_DTYPE.itemsize, dtype=torch.uint8).pin_memory()
                h_flags = torch.zeros(n, dtype=torch.uint8).pin_memory()
                d_flags = torch.zeros(n, dtype=torch.uint8, device=dev)

                def through_host():
                    h_fw.copy_(d_hits, non_blocking=True)
                    torch.cuda.synchronize()
                    d_flags.copy_(h_flags, non_blocking=True)
                    torch.cuda.synchronize()
                emit(nflows, "d_through_host", [wall(through_host) for _ in range(a.windows)],
                     clock="wall time: D2H of d_fw into pinned memory, H2D of one flag byte per packet; no host lookup")

                # an add of n new flows: both launches, on a table that holds only its own flows again each time
                if 2 * nflows - nflows >= n:
                    d_rem = torch.zeros(n, dtype=torch.int64, device=dev)
                    ws = []
                    for _ in range(a.windows):
                        total, runs = 0.0, 0
                        while total < a.window * 1e3 and runs < 200:
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            ct.add_device(d_fresh, d_inc, n, T0 + 3, d_res)
                            e1.record()
                            e1.synchronize()
                            total += e0.elapsed_time(e1)
                            runs += 1
                            ct.evict_device(d_fresh, n, T0 + 3, d_rem, force=True)
                            if ct.should_compact():
                                ct.compact()
                        ws.append(total * 1e3 / runs)
                    emit(nflows, "add_new", ws, launches="claim, settle", new_flows=n)
                ct.compact()
                ws = []
                for _ in range(a.windows):
                    t0 = time.perf_counter()
                    ct.compact()
                    ws.append((time.perf_counter() - t0) * 1e6)
                emit(nflows, "compact", ws, clock="wall time of the blocking call, one call per window", slots=ct.count()[2])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
