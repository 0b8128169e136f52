"""What the RX batch report (neb_rx_report_batch) costs on a device-resident receive batch, beside the
resolve and the open it follows, the host loop it replaces and the download it saves.

Workload: 65 536 wire packets of 1364 bytes, arriving round-robin over their tunnels, every tunnel from
one source, in three shapes:

  1_tunnel        one tunnel holds every packet
  4096_tunnels    4096 tunnels, 16 packets each
  4096_and_relay  the same, and every 16th packet is a Message/Relay packet of a relay tunnel, over 64
                  relay indexes

Measures, per shape:

  a_report      neb_rx_report_batch alone (device events around a run of calls)
  b_pair        neb_rx_resolve_batch + neb_rx_open_wire_batch on freshly sealed packets (AES-256-GCM),
  b_reported    against the same pair with the report behind it on the same stream, alternating step by
                step; delta_us is the difference of the medians. Real opens, so only the two shapes
                without relay packets
  c_host_form   neb_rx_report_batch_host's C entry point on one thread, outputs allocated once (wall time)
  d_download    what the caller reads back today, pk + status + src for every packet (40 B x packets),
                against the report: the counts first, then nruns run records, the relay and work
                records and the metrics (wall time, device to pinned host memory, each step ended by a
                synchronise)

a, c and d run on statuses and headers written directly (every packet opened): the report reads
nothing else. a, c and d: the median over windows of at least --window seconds of timed work; b: the
median, the least and the most over --steps steps per form. Before timing the device form must equal
the host form.

  python tools/rx_report_bench.py --out profiles/rx_report/bench.jsonl
  rocprofv3 --kernel-trace --stats ... -- python tools/rx_report_bench.py --measures a --window 0.02 --windows 1
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recv_plan_bench as RB  # noqa: E402  (its keys, sealed batches and timers)
from nebula_amd import _lib as L  # noqa: E402
from nebula_amd.noiseutil import Engine  # noqa: E402

N, WIRE = 65536, RB.WIRE
SHAPES = {"1_tunnel": (1, 0), "4096_tunnels": (4096, 0), "4096_and_relay": (4096, 64)}


class Synthetic:
    """A finished batch written directly: packet i belongs to tunnel i % ntun (key_id = the tunnel),
    status OK, a Message header; with relay indexes every 16th packet is a Message/Relay packet of
    tunnel ntun, its index i / 16 % nrelay."""

    def __init__(self, torch, dev, ntun, nrelay):
        self.torch, self.dev = torch, dev
        i = np.arange(N)
        relay = (i % 16 == 15) if nrelay else np.zeros(N, bool)
        pk = np.zeros(N, L.RX_PACKET_DTYPE)
        pk["off"], pk["len"], pk["key_id"] = i * WIRE, WIRE, np.where(relay, ntun, i % ntun)
        hdr = RB.headers(np.where(relay, 0x500 + i // 16 % max(nrelay, 1), 0x20000000 + i % ntun), i + 1)
        hdr[relay, 1] = 1
        frm = np.zeros(N, L.UDP_ADDR_DTYPE)
        frm["addr"][:, :4] = [0x20, 0x01, 0x0d, 0xb8]
        frm["addr"][:, 12:16] = pk["key_id"].astype(">u4").reshape(-1, 1).view(np.uint8)
        frm["port"], frm["family"] = 4242, 6
        self.pk, self.status, self.frm, self.hdr = pk, np.zeros(N, np.int32), frm, hdr
        src = np.zeros(N, L.RX_SOURCE_DTYPE)
        src["addr"], src["family"] = frm["addr"], 6
        self.src = src
        self.arena = torch.zeros(N * WIRE + 64, dtype=torch.uint8, device=dev)
        self.arena[:N * WIRE].view(N, WIRE)[:, :16] = self.up(hdr).view(N, 16)
        self.d_pk, self.d_status, self.d_frm = self.up(pk), self.up(self.status), self.up(frm)
        self.out = Outputs(torch, dev)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev)

    def host_args(self):
        vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
        arena = np.zeros(N * WIRE, np.uint8)
        arena.reshape(N, WIRE)[:, :16] = self.hdr
        o = {"runs": np.zeros(N, L.RX_RUN_DTYPE), "relay_used": np.zeros(N, L.RX_RELAY_USED_DTYPE),
             "work": np.zeros(N, L.RX_WORK_DTYPE), "metrics": np.zeros(16, np.uint64), "counts": np.zeros(4, np.uint32)}
        keep = (arena, self.pk, self.status, self.frm)
        return o, keep, (vp(self.pk), vp(self.status), N, vp(arena), arena.nbytes, vp(self.frm), None, N, 0, vp(o["runs"]),
                         vp(o["relay_used"]), vp(o["work"]), vp(o["metrics"]), vp(o["counts"]))


class Outputs:
    def __init__(self, torch, dev):
        z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=dev)  # noqa: E731
        self.runs, self.relay_used, self.work = z(N * 40), z(N * 8), z(N * 8)
        self.metrics, self.counts = z(16 * 8), z(16)


def report_call(eng, d_pk, d_status, d_arena, d_frm, out, stream):
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    args = (eng.handle, p(d_pk), p(d_status), N, p(d_arena), p(d_frm), None, N, 0, p(out.runs), p(out.relay_used), p(out.work),
            p(out.metrics), p(out.counts), stream)
    return lambda: L.lib().neb_rx_report_batch(*args)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed work per window, at least")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30, help="b: timed steps per form")
    ap.add_argument("--measures", default="a,b,c,d")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("rx_report_bench: no GPU (this tool measures on the device only)")
    measures = a.measures.split(",")
    lines = []
    dev = torch.device("cuda", 0)

    def emit(shape, measure, us, **more):
        lines.append({"tool": "rx_report_bench", "measure": measure, "shape": shape, "packets": N, "wire_bytes": WIRE,
                      "median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                      "samples": len(us), "device": torch.cuda.get_device_name(0), "build": L.lib().neb_build_id().decode(),
                      **more})
        print(json.dumps(lines[-1]), flush=True)

    for shape in a.shapes.split(","):
        ntun, nrelay = SHAPES[shape]
        with Engine(0, ntun + 64) as eng:
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            syn = Synthetic(torch, dev, ntun, nrelay)
            call = report_call(eng, syn.d_pk, syn.d_status, syn.arena, syn.d_frm, syn.out, stream)
            o, keep, hargs = syn.host_args()
            L.check(L.lib().neb_rx_report_batch_host(*hargs), "neb_rx_report_batch_host")
            L.check(call(), "neb_rx_report_batch")
            torch.cuda.synchronize()
            counts = syn.out.counts.cpu().numpy().view(np.uint32)[:4]
            assert counts.tolist() == o["counts"].tolist(), (counts, o["counts"])
            for name, cnt, item in (("runs", counts[0], 40), ("relay_used", counts[2], 8), ("work", counts[3], 8), ("metrics", 16, 8)):
                got = getattr(syn.out, name).cpu().numpy()[:int(cnt) * item]
                assert got.tobytes() == o[name][:int(cnt)].tobytes(), (shape, name)
            shape_info = dict(tunnels=int(counts[1]), runs=int(counts[0]), relay_used=int(counts[2]), work=int(counts[3]))
            timer = RB.Case.timed_launches
            holder = type("T", (), {"torch": torch})()
            if "a" in measures:
                res = [timer(holder, call, a.window) for _ in range(a.windows)]
                emit(shape, "a_report", [u for u, _ in res], window_s=a.window, launches_per_window=res[-1][1], **shape_info)
            if "c" in measures:
                emit(shape, "c_host_form", RB.wall(lambda: L.lib().neb_rx_report_batch_host(*hargs), a.window, a.windows),
                     window_s=a.window, clock="wall time of the calling thread on the GPU machine's host, outputs allocated once",
                     **shape_info)
            if "d" in measures:
                def pinned(nbytes):
                    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8).pin_memory()
                d_src = syn.up(syn.src)
                per_packet = [(syn.d_pk, pinned(N * 16)), (syn.d_status, pinned(N * 4)), (d_src, pinned(N * 20))]
                h_counts, h_metrics = pinned(16), pinned(128)
                h_runs, h_used, h_work = pinned(N * 40), pinned(N * 8), pinned(N * 8)

                def today():
                    for d, h in per_packet:
                        h.copy_(d, non_blocking=True)
                    torch.cuda.synchronize()

                def with_report():
                    h_counts.copy_(syn.out.counts, non_blocking=True)
                    torch.cuda.synchronize()
                    c = h_counts.numpy().view(np.uint32)
                    for d, h, cnt, item in ((syn.out.runs, h_runs, c[0], 40), (syn.out.relay_used, h_used, c[2], 8),
                                            (syn.out.work, h_work, c[3], 8), (syn.out.metrics, h_metrics, 16, 8)):
                        if cnt:
                            h[:int(cnt) * item].copy_(d[:int(cnt) * item], non_blocking=True)
                    torch.cuda.synchronize()
                emit(shape, "d_download", RB.wall(today, a.window, a.windows), what="pk_status_src", bytes=N * 40, window_s=a.window,
                     clock="wall time: D2H into pinned memory, ended by a synchronise")
                emit(shape, "d_download", RB.wall(with_report, a.window, a.windows), what="report",
                     bytes=int(16 + 128 + counts[0] * 40 + counts[2] * 8 + counts[3] * 8), window_s=a.window,
                     clock="wall time: counts, a synchronise, then the records, a synchronise")
            if "b" in measures and not nrelay:
                RB.NTUN = ntun
                keys = RB.Keys(eng, L.ALG_AESGCM)
                case = RB.Case(eng, L.ALG_AESGCM, keys, "65536x1")
                try:
                    assert case.n == N
                    _, _, _, pair = case.bare()
                    frm = np.zeros(N, L.UDP_ADDR_DTYPE)
                    frm["addr"], frm["port"], frm["family"] = case.src["addr"], 4242, 6
                    out = Outputs(torch, dev)
                    rep = report_call(eng, case.d_pk, case.d_status, case.arena, case.up(frm), out, stream)
                    got = {"b_pair": [], "b_reported": []}
                    for step in range(a.steps + 3):
                        for form in got:
                            case.prepare()
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            pair()
                            if form == "b_reported":
                                rep()
                            e1.record()
                            e1.synchronize()
                            assert (case.d_status == 0).all().item()
                            if step >= 3:
                                got[form].append(e0.elapsed_time(e1) * 1e3)
                    c = out.counts.cpu().numpy().view(np.uint32)[:4].tolist()
                    assert c == [ntun, ntun, 0, 0], c
                    base = statistics.median(got["b_pair"])
                    emit(shape, "b_pair", got["b_pair"])
                    emit(shape, "b_reported", got["b_reported"], delta_us=round(statistics.median(got["b_reported"]) - base, 2),
                         runs=c[0], tunnels=c[1])
                finally:
                    case.close()
                    keys.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
