"""What the TX send plan (neb_tx_send_plan) costs on the device-resident wires of a TX batch, beside
the batch it follows and the host loop it replaces.

Workload: --reads IPv4/TCP TSO superpackets of 45 x 1448 B (default 1456: 65 520 wires; DESIGN §3.5's
shape), AES-256-GCM, sealed once by neb_tx_seal_batch / neb_tx_seal_via_batch; the plan reads their
wires where the batch left them. Cases (targets:relays): 1:0 one tunnel, 4096:0 4096 tunnels sent
directly, 4096:64 4096 targets through 64 relays. A v4 socket, max_segments 63, chunk_packets 128 and
0. Measures, per case and chunk size:

  a_plan          neb_tx_send_plan alone (device events around a run of calls)
  b_batch         the TX batch alone, against
  b_batch_plan    the TX batch with the plan behind it on the same stream, alternating step by step;
                  delta_us in the second line is the difference of the medians
  c_host_form     neb_tx_send_plan_host's C entry point on one thread over the downloaded wires, into
                  output arrays allocated once (wall time of the calling thread)
  d_download      the wires, their statuses and the count copied to pinned host memory (wall time): what
                  the host form needs first when the wires live on the device

Every figure is the median over windows of at least --window seconds of timed work. Before timing the
device form must equal the host form.

  python tools/send_plan_bench.py --out profiles/send_plan/bench.jsonl
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from bench import tso_superpackets  # noqa: E402
from nebula_amd import _lib as L  # noqa: E402
from nebula_amd.inside import (TX_PACKET_DTYPE, TX_TUNNEL_DTYPE, TX_WIRE_DTYPE, DeviceSendPlan, DeviceTxBatch,  # noqa: E402
                               send_plan_host)
from nebula_amd.noiseutil import Engine  # noqa: E402

MSS, PER = 1448, 45
SEG = 40 + MSS
DIRECT, VIA = SEG + 32, SEG + 64


class Case:
    def __init__(self, eng, nreads, ntargets, nrelays, seed=1):
        import torch

        self.torch, self.eng, self.alg = torch, eng, L.ALG_AESGCM
        self.ntargets, self.nrelays = ntargets, nrelays
        rng = np.random.default_rng(seed)
        nt = nrelays + ntargets
        keys = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        out = (C.c_void_p * nt)()
        L.check(L.lib().neb_cipher_create_batch(eng.handle, self.alg, keys.ctypes.data_as(C.c_void_p), nt, out),
                "neb_cipher_create_batch")
        self.ciphers = [C.c_void_p(h) for h in out]
        kid = np.array([L.lib().neb_cipher_key_id(c) for c in self.ciphers], np.uint32)
        # tunnels 0..nrelays-1 are the relays, the targets follow; target t goes through relay t % nrelays
        tun = np.zeros(nt, TX_TUNNEL_DTYPE)
        tun["message_counter"] = 2 + 1000 * np.arange(nt)
        tun["key_id"], tun["remote_index"] = kid, 0x9000 + np.arange(nt)
        via = None
        self.remote = np.zeros(nt, L.UDP_ADDR_DTYPE)
        j = np.arange(nt)
        self.remote["family"], self.remote["port"] = 4, 4242
        self.remote["addr"][:, 0], self.remote["addr"][:, 1] = 10, 1 + j // 65536
        self.remote["addr"][:, 2], self.remote["addr"][:, 3] = (j // 256) % 256, j % 256
        if nrelays:
            via = np.zeros(nt, L.RELAY_ROUTE_DTYPE)
            via["tunnel"] = L.RELAY_NONE
            via["tunnel"][nrelays:] = np.arange(ntargets) % nrelays
            via["remote_index"][nrelays:] = 0x7000 + np.arange(ntargets)
            self.remote[nrelays:] = np.zeros(1, L.UDP_ADDR_DTYPE)[0]  # no valid remote: reached through the relay only
        self.via = via
        arena, nsp, size, stride, per = tso_superpackets(PER * nreads, MSS)
        assert nsp == nreads and per == PER
        self.nreads, self.nw = nsp, nsp * per
        pk = np.zeros(nsp, TX_PACKET_DTYPE)
        read_tun = (nrelays + (np.arange(nsp) * 7 + 3) % ntargets).astype(np.uint32)
        for i in range(nsp):
            pk[i] = (i * stride, size, read_tun[i], 1, 1, 40, MSS, 20, 16, 0)
        self.pk = pk
        hint = int(kid[nrelays]) if ntargets == 1 else L.KEYS_MIXED
        self.batch = DeviceTxBatch(eng, self.alg, tun, pk, arena, self.nw * (VIA if nrelays else DIRECT), self.nw, hint, via=via)
        self.plans = {}

    def plan(self, chunk):
        if chunk not in self.plans:
            self.plans[chunk] = DeviceSendPlan(self.batch, self.remote, True, 63, chunk)
        return self.plans[chunk]

    def check(self, chunk):
        """The batch seals every wire; the device plan equals the host form's. Returns the host inputs."""
        t = self.torch
        self.batch.seal()
        self.plan(chunk).plan()
        t.cuda.synchronize()
        r, got = self.batch.result(), self.plan(chunk).result()
        assert len(r.wires) == self.nw and (r.wire_status == 0).all()
        want = send_plan_host(r.wires, r.wire_status, self.pk, self.via, self.remote, True, 63, chunk)
        for k in ("iov", "entries", "wire_entry", "send_status"):
            assert getattr(got, k).tobytes() == getattr(want, k).tobytes(), k
        assert (got.send_status == 0).all()
        return r, want

    def timed_launches(self, fn, window):
        """us per call of an enqueue-only call: device events around a run long enough for the window."""
        t = self.torch
        for _ in range(20):
            fn()
        t.cuda.synchronize()
        count = 200
        while True:
            a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(count):
                fn()
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= window * 1e3:
                return ms * 1e3 / count, count
            count = int(count * max(2.0, 1.2 * window * 1e3 / max(ms, 1e-3)))

    def close(self):
        for c in self.ciphers:
            L.lib().neb_cipher_destroy(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1456)
    ap.add_argument("--cases", default="1:0,4096:0,4096:64", help="targets:relays, comma separated")
    ap.add_argument("--chunks", default="128,0")
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed work per window, at least")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--measures", default="a,b,c,d")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("send_plan_bench: no GPU (this tool measures on the device only)")
    cases = [tuple(int(x) for x in c.split(":")) for c in a.cases.split(",")]
    chunks = [int(x) for x in a.chunks.split(",")]
    measures = a.measures.split(",")
    lines = []

    def emit(case, measure, chunk, windows_us, **more):
        lines.append({"tool": "send_plan_bench", "measure": measure, "reads": case.nreads, "wires": case.nw,
                      "targets": case.ntargets, "relays": case.nrelays, "max_segments": 63, "chunk_packets": chunk,
                      "median_us": round(statistics.median(windows_us), 2), "windows_us": [round(x, 2) for x in windows_us],
                      "window_s": a.window, "device": torch.cuda.get_device_name(0), "build": L.lib().neb_build_id().decode(),
                      **more})
        print(json.dumps(lines[-1]), flush=True)

    with Engine(0, max(t + r for t, r in cases) + 64) as eng:
        for ntargets, nrelays in cases:
            case = Case(eng, a.reads, ntargets, nrelays)
            try:
                for chunk in chunks:
                    r, want = case.check(chunk)
                    shape = {"iovecs": len(want.iov), "entries": len(want.entries)}
                    sp = case.plan(chunk)
                    if "a" in measures:
                        res = [case.timed_launches(sp.plan, a.window) for _ in range(a.windows)]
                        emit(case, "a_plan", chunk, [u for u, _ in res], launches_per_window=res[-1][1], **shape)
                    if "b" in measures:  # alternating, step by step, until each form has its windows
                        forms = {"b_batch": False, "b_batch_plan": True}
                        done, acc, warm = {f: [] for f in forms}, {f: [0.0, 0] for f in forms}, 3
                        while any(len(v) < a.windows for v in done.values()):
                            for f, with_plan in forms.items():
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                torch.cuda.synchronize()
                                e0.record()
                                case.batch.seal()
                                if with_plan:
                                    sp.plan()
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
                        base = statistics.median(done["b_batch"][:a.windows])
                        emit(case, "b_batch", chunk, done["b_batch"][:a.windows])
                        emit(case, "b_batch_plan", chunk, done["b_batch_plan"][:a.windows],
                             delta_us=round(statistics.median(done["b_batch_plan"][:a.windows]) - base, 2), **shape)
                if "c" in measures:
                    vp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
                    n = case.nw
                    o_iov, o_ent = np.zeros(n, L.SEND_IOV_DTYPE), np.zeros(n, L.SEND_ENTRY_DTYPE)
                    o_we, o_st = np.zeros(n, np.uint32), np.zeros(n, np.int32)
                    ni, ne = C.c_uint32(0), C.c_uint32(0)
                    wires, wst = np.ascontiguousarray(r.wires), np.ascontiguousarray(r.wire_status)
                    for chunk in chunks:
                        ws = []
                        for _ in range(a.windows):
                            t0, calls = time.perf_counter(), 0
                            while time.perf_counter() - t0 < a.window:
                                L.check(L.lib().neb_tx_send_plan_host(vp(wires), vp(wst), n, vp(case.pk), len(case.pk), vp(case.via),
                                                                      vp(case.remote), len(case.remote), 1, 63, chunk, vp(o_iov),
                                                                      C.byref(ni), vp(o_ent), C.byref(ne), vp(o_we), vp(o_st)),
                                        "neb_tx_send_plan_host")
                                calls += 1
                            ws.append((time.perf_counter() - t0) * 1e6 / calls)
                        emit(case, "c_host_form", chunk, ws, entries=ne.value,
                             clock="wall time of the calling thread on the GPU box's host, outputs allocated once")
                if "d" in measures:
                    b = case.batch
                    h_w = torch.empty(b.wires.numel(), dtype=torch.uint8).pin_memory()
                    h_s = torch.empty(b.wire_status.numel(), dtype=torch.int32).pin_memory()
                    h_n = torch.empty(1, dtype=torch.int32).pin_memory()
                    ws = []
                    for _ in range(a.windows):
                        t0, calls = time.perf_counter(), 0
                        while time.perf_counter() - t0 < a.window:
                            h_w.copy_(b.wires, non_blocking=True)
                            h_s.copy_(b.wire_status, non_blocking=True)
                            h_n.copy_(b.nwires, non_blocking=True)
                            torch.cuda.synchronize()
                            calls += 1
                        ws.append((time.perf_counter() - t0) * 1e6 / calls)
                    emit(case, "d_download", -1, ws, bytes=case.nw * (TX_WIRE_DTYPE.itemsize + 4) + 4,
                         clock="wall time: D2H of wires, statuses and the count into pinned memory")
            finally:
                case.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
