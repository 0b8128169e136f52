#!/usr/bin/env python3
"""Receive coalescer (neb_rx_coalesce_batch) on a device-resident batch: 64 Ki opened TCP packets of
a 1300-byte MTU, for 1 tunnel / 1 flow and for 4096 tunnels x 4 flows in arrival order.

Per shape, one JSON line to profiles/coalesce/bench.jsonl:
  call_us            the whole call, hipEvents around it (median of --steps after --warmup)
  gather_us          the gather kernel alone (neb_time_next_kernel binds the pair to that dispatch)
  copy_us            a device-to-device copy of the same number of bytes, same process
  gather_over_copy   their ratio
  tun_gibs           GiB/s of TUN bytes (the bytes written to the output arena) over the whole call
  rx_open_us         neb_rx_open_batch (replay windows on the device) of a batch of the same size
  stages_us          per-stage kernel time, with --stages: this script runs itself once per shape as
                     a child under `rocprofv3 --kernel-trace --stats` and sums the kernels by stage

  python tools/coalesce_bench.py [--steps 30] [--warmup 5] [--stages] [--n 65536]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nebula_amd import Engine, _lib as L  # noqa: E402

MTU = 1300
STRIDE = 1344  # a wire slot: header 16 + packet + tag 16, rounded to 64; the plaintext sits at +16
GIB = float(1 << 30)
STAGES = (("parse", ("co_parse",)), ("sort", ("sort", "radix", "onesweep", "co_epoch_key")),
          ("scan", ("scan",)), ("flows", ("co_lane_key", "co_pred")), ("links_chains", ("co_link", "co_chain", "co_jump")),
          ("emit", ("co_member", "co_slot", "co_emit", "co_result")), ("gather", ("co_gather",)))


def build(shape: str, n: int):
    """-> (plain records, arena): IPv4/TCP segments of MTU bytes, DF set, ACK only, seq contiguous per flow."""
    if shape == "1x1":
        tun = np.zeros(n, np.int64)
        flow = np.zeros(n, np.int64)
        k = np.arange(n, dtype=np.int64)  # position within the flow
        ctr = k + 1
    else:  # 4096 tunnels x 4 flows; arrival: round-robin over the tunnels, one flow's burst of 4 per visit
        ntun, nfl, burst = 4096, 4, max(1, n // (4096 * 4))
        i = np.arange(n, dtype=np.int64)
        visit, b = i // burst, i % burst
        tun = visit % ntun
        flow = (visit // ntun) % nfl
        rnd = visit // (ntun * nfl)
        k = rnd * burst + b
        ctr = (flow + nfl * rnd) * burst + b + 1  # per tunnel: the order its packets were sent in
    pay = MTU - 40
    pk = np.zeros((n, STRIDE), np.uint8)
    body = pk[:, 16:16 + MTU]
    body[:, 0] = 0x45
    body[:, 2:4] = np.array([MTU >> 8, MTU & 0xFF], np.uint8)
    body[:, 4] = (k >> 8) & 0xFF
    body[:, 5] = k & 0xFF
    body[:, 6] = 0x40
    body[:, 8] = 64
    body[:, 9] = 6
    body[:, 12:16] = np.stack([np.full(n, 10), (tun >> 8) & 0xFF, tun & 0xFF, np.full(n, 1)], 1).astype(np.uint8)
    body[:, 16:20] = np.array([10, 200, 0, 1], np.uint8)
    sport = 1000 + flow
    body[:, 20] = sport >> 8
    body[:, 21] = sport & 0xFF
    body[:, 22:24] = np.array([0, 80], np.uint8)
    seq = (1000 + k * pay) & 0xFFFFFFFF
    for j in range(4):
        body[:, 24 + j] = (seq >> (24 - 8 * j)) & 0xFF
    body[:, 32] = 5 << 4
    body[:, 33] = 0x10
    body[:, 34:36] = np.array([0x10, 0], np.uint8)
    body[:, 40:] = (np.arange(pay, dtype=np.int64)[None, :] * 7 + k[:, None]).astype(np.uint8)
    plain = np.zeros(n, L.PLAIN_PACKET_DTYPE)
    plain["off"] = np.arange(n, dtype=np.uint64) * np.uint64(STRIDE) + np.uint64(16)
    plain["len"] = MTU
    plain["epoch"] = (tun + 1).astype(np.uint64)
    plain["counter"] = ctr.astype(np.uint64)
    return plain, pk.reshape(-1)


def median_us(ms):
    return round(statistics.median(ms) * 1e3, 2)


def run_shape(eng, shape, n, steps, warmup, child=False):
    import torch

    dev = torch.device("cuda", eng.device)
    plain, arena = build(shape, n)
    up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1)).to(dev)  # noqa: E731
    d_plain, d_in = up(plain), up(arena)
    cap = n * ((MTU + 15) & ~15)
    d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_writes = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_nw = torch.zeros(1, dtype=torch.int32, device=dev)
    d_pw = torch.zeros(n, dtype=torch.int32, device=dev)
    d_ps = torch.zeros(n, dtype=torch.int32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = torch.cuda.current_stream().cuda_stream
    lib = L.lib()

    def call():
        L.check(lib.neb_rx_coalesce_batch(eng.handle, p(d_plain), n, p(d_in), p(d_out), cap, p(d_writes), n, p(d_nw),
                                          p(d_pw), p(d_ps), 3, C.c_void_p(stream)), "neb_rx_coalesce_batch")

    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    call_ms, gather_ms, copy_ms = [], [], []
    for it in range(warmup + steps):
        a, b, g0, g1 = ev(), ev(), ev(), ev()
        g0.record(), g1.record()  # create the underlying hipEvents before they are bound
        torch.cuda.synchronize()
        if not child:
            L.check(lib.neb_time_next_kernel(C.c_void_p(g0.cuda_event), C.c_void_p(g1.cuda_event)), "time_next_kernel")
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            call_ms.append(a.elapsed_time(b))
            if not child:
                gather_ms.append(g0.elapsed_time(g1))
    if child:
        return None
    writes = d_writes.cpu().numpy().view(L.TUN_WRITE_DTYPE)[:int(d_nw.item())]
    assert (d_ps.cpu().numpy() == 0).all()
    tun_bytes = int(writes["len"].astype(np.int64).sum())
    src = torch.empty(tun_bytes, dtype=torch.uint8, device=dev)
    dst = torch.empty(tun_bytes, dtype=torch.uint8, device=dev)
    for it in range(warmup + steps):
        a, b = ev(), ev()
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        if it >= warmup:
            copy_ms.append(a.elapsed_time(b))
    name = lib.neb_time_last_kernel().decode()
    return {"shape": shape, "packets": n, "mtu": MTU, "writes": int(len(writes)),
            "segments_per_write": round(n / max(len(writes), 1), 2), "tun_bytes": tun_bytes, "steps": steps,
            "warmup": warmup, "call_us": median_us(call_ms), "gather_us": median_us(gather_ms),
            "gather_kernel": name.split("(")[0], "copy_us": median_us(copy_ms),
            "gather_over_copy": round(statistics.median(gather_ms) / statistics.median(copy_ms), 2),
            "tun_gibs": round(tun_bytes / (statistics.median(call_ms) * 1e-3) / GIB, 1),
            "gather_gibs": round(tun_bytes / (statistics.median(gather_ms) * 1e-3) / GIB, 1),
            "copy_gibs": round(tun_bytes / (statistics.median(copy_ms) * 1e-3) / GIB, 1)}


def rx_open_us(eng, n, nkeys, steps, warmup):
    """neb_rx_open_batch of n 1300-byte packets of nkeys tunnels (what bench.py --mode rx-device times)."""
    import torch

    from nebula_amd.batch import DeviceBatch, install_keys
    from nebula_amd.connection_state import Bits, DeviceWindows, ReplayWindow, rx_open_batch_device
    from nebula_amd.workload import make_batch

    b = make_batch(L.ALG_AESGCM, n, nkeys, name="coalesce-bench")
    ciphers = install_keys(eng, b)
    db = DeviceBatch(eng, b, ciphers)
    pt, base = db.arena.clone(), db.desc_host.copy()
    dw = DeviceWindows(eng, eng.max_keys, ReplayWindow)
    for c in ciphers:
        w = Bits(ReplayWindow)
        dw.load(c.key_id, w)
        w.destroy()
    ms = []
    for it in range(warmup + steps):
        d = base.copy()
        d["counter"] = d["counter"] + np.uint64(it * b.n)
        db.desc.copy_(torch.from_numpy(d.view(np.uint8)))
        db.arena.copy_(pt)
        db.seal()
        torch.cuda.synchronize()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rx_open_batch_device(eng, b.alg, dw, db.desc, db.arena, db.status, db.key_hint,
                             torch.cuda.current_stream().cuda_stream)
        e.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(a.elapsed_time(e))
    dw.destroy()
    for c in ciphers:
        c.destroy()
    return median_us(ms)


def stage_times(shape, n):
    """Run this script as a child under rocprofv3 and sum its kernel stats by stage (µs per call)."""
    steps = 5
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "-o", "co", "--",
               sys.executable, os.path.abspath(__file__), "--child", shape, "--n", str(n), "--steps", str(steps),
               "--warmup", "0"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"error": (r.stderr or r.stdout)[-400:]}
        files = glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv"}
        out = {s: 0.0 for s, _ in STAGES}
        out["other"] = 0.0
        for row in csv.DictReader(open(files[0])):
            name, total = row["Name"], float(row["TotalDurationNs"])
            for s, pats in STAGES:
                if any(x in name for x in pats):
                    out[s] += total
                    break
            else:
                out["other"] += total
        return {k: round(v / steps / 1e3, 2) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--no-rx", action="store_true")
    ap.add_argument("--child", default=None, help="internal: run one shape's calls only (under the profiler)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coalesce", "bench.jsonl"))
    args = ap.parse_args()
    if args.child:
        eng = Engine(0, max_keys=16)
        run_shape(eng, args.child, args.n, args.steps, args.warmup, child=True)
        eng.close()
        return
    stages = {s: stage_times(s, args.n) for s in ("1x1", "4096x4")} if args.stages else {}
    eng = Engine(0, max_keys=8192)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        for shape, nkeys in (("1x1", 1), ("4096x4", 4096)):
            res = run_shape(eng, shape, args.n, args.steps, args.warmup)
            if not args.no_rx:
                res["rx_open_us"] = rx_open_us(eng, args.n, nkeys, max(args.steps // 2, 10), 3)
            if shape in stages:
                res["stages_us"] = stages[shape]
            line = json.dumps(res)
            print(line, flush=True)
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
