"""Relay forwarding on a device-resident receive batch: neb_relay_forward_batch (one call) against
the same work composed by a caller from the other entry points (neb_rx_open_wire_batch, statuses
to the host, counters and headers on the host, upload, neb_seal_batch).

Workload: --n relay packets (default 64 Ki) whose AD is 1348 B (outer header 16 + a 1332-B inner wire
packet, as workload.relay_batch) plus the 16-B tag = 1364 wire bytes, forwarded 1 key -> 1 key and
4096 -> 4096. Every step gets fresh inbound counters (its packets are re-sealed on the device,
outside the timed window) so the windows accept them. Both forms are timed in one process,
alternating, with a host clock around work that ends in a device synchronize; GiB/s of wire bytes
from the median. Before timing, both forms run on the same input and must leave the same bytes.

  python tools/relay_forward_bench.py --out profiles/relay_fwd/bench.jsonl
  rocprofv3 --kernel-trace --stats ... -- python tools/relay_forward_bench.py --forms call --steps 5
  (then tools/trace_sched.py on the trace: the plan's kernels are neb::relay_* and the hipcub sort /
  scan-by-key between them)
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
from nebula_amd.connection_state import Bits, DeviceWindows, rx_open_wire_batch_device  # noqa: E402
from nebula_amd.inside import TX_TUNNEL_DTYPE  # noqa: E402
from nebula_amd.noiseutil import Engine  # noqa: E402
from nebula_amd.relay import relay_forward_batch_device  # noqa: E402

AD, WIRE, STRIDE = 1348, 1364, 1408


def headers(remote_index, counters):
    """header.Encode(1, Message, MessageRelay, remote_index, counter) for arrays -> (n, 16) uint8"""
    h = np.zeros((len(counters), 16), np.uint8)
    h[:, 0], h[:, 1] = 0x11, 1
    h[:, 4:8] = np.asarray(remote_index, ">u4").reshape(-1, 1).view(np.uint8)
    h[:, 8:16] = np.asarray(counters, ">u8").reshape(-1, 1).view(np.uint8)
    return h


def relay_desc(off, counters, key_ids):
    d = np.zeros(len(off), L.DESC_DTYPE)
    d["aad_off"] = off
    d["src_off"] = d["dst_off"] = off + np.uint64(AD)
    d["counter"], d["aad_len"], d["key_id"] = counters, AD, key_ids
    return d


class Case:
    def __init__(self, eng, alg, n, nkeys, seed=1):
        import torch

        self.torch, self.eng, self.alg, self.n, self.nkeys = torch, eng, alg, n, nkeys
        self.dev = torch.device("cuda", eng.device)
        rng = np.random.default_rng(seed)
        keys = rng.integers(0, 256, (2 * nkeys, 32), dtype=np.uint8)
        out = (C.c_void_p * (2 * nkeys))()
        L.check(L.lib().neb_cipher_create_batch(eng.handle, alg, keys.ctypes.data_as(C.c_void_p), 2 * nkeys, out),
                "neb_cipher_create_batch")
        self.ciphers = [C.c_void_p(h) for h in out]
        kid = np.array([L.lib().neb_cipher_key_id(c) for c in self.ciphers], np.uint32)
        self.in_kid, self.out_kid = kid[:nkeys], kid[nkeys:]
        i = np.arange(n)
        self.in_tun = (i % nkeys).astype(np.uint32)           # inbound tunnels interleaved
        self.route_tun = ((i * 7 + 3) % nkeys).astype(np.uint32)
        self.place = (i // nkeys).astype(np.uint64)            # a packet's place among its inbound tunnel's
        self.per_tun = -(-n // nkeys)
        self.off = (i * STRIDE).astype(np.uint64)
        self.hint_in = int(self.in_kid[0]) if nkeys == 1 else L.KEYS_MIXED
        self.hint_out = int(self.out_kid[0]) if nkeys == 1 else L.KEYS_MIXED
        up = self.up
        self.arena = torch.from_numpy(rng.integers(0, 256, n * STRIDE, dtype=np.uint8)).to(self.dev)
        pk = np.zeros(n, L.RX_PACKET_DTYPE)
        pk["off"], pk["len"], pk["key_id"] = self.off, WIRE, self.in_kid[self.in_tun]
        rt = np.zeros(n, L.RELAY_ROUTE_DTYPE)
        rt["tunnel"], rt["remote_index"] = self.route_tun, 0x7000 + self.route_tun
        self.routes = rt
        self.tun0 = np.zeros(nkeys, TX_TUNNEL_DTYPE)
        self.tun0["key_id"], self.tun0["remote_index"] = self.out_kid, 0x9000 + np.arange(nkeys)
        self.d_pk, self.d_rt, self.d_tun = up(pk), up(rt), up(self.tun0)
        self.d_status = torch.zeros(n, dtype=torch.int32, device=self.dev)
        self.d_fwd = torch.zeros(n, dtype=torch.int32, device=self.dev)
        self.d_sub = torch.zeros(n, dtype=torch.int32, device=self.dev)
        self.d_desc = torch.zeros(n * L.DESC_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        self.d_hdr = torch.zeros((n, 16), dtype=torch.uint8, device=self.dev)
        self.rows = self.arena.view(n, STRIDE)
        self.dw = DeviceWindows(eng, eng.max_keys, 8192)
        for k in self.in_kid:
            self.dw.load(int(k), Bits(8192))
        self.step = 0
        self.tun_host = self.tun0.copy()  # the composed form keeps the counters on the host

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(self.dev)

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def prepare(self):
        """Untimed: this step's inbound packets — fresh counters in the headers, sealed on the device."""
        self.step += 1
        ctr = np.uint64(self.step * self.per_tun) + self.place + np.uint64(1)
        self.rows[:, :16] = self.up(headers(0x1000 + self.in_tun, ctr)).view(self.n, 16)
        d = self.up(relay_desc(self.off, ctr, self.in_kid[self.in_tun]))
        L.check(L.lib().neb_seal_batch(self.eng.handle, self.alg, C.c_void_p(d.data_ptr()), self.n,
                                       C.c_void_p(self.arena.data_ptr()), C.c_void_p(self.d_sub.data_ptr()),
                                       self.hint_in, self.stream()), "neb_seal_batch")
        self.torch.cuda.synchronize()

    def one_call(self):
        relay_forward_batch_device(self.eng, self.alg, self.dw, self.d_pk, self.d_rt, self.d_tun, self.arena,
                                   self.d_status, self.d_fwd, self.hint_in)
        self.torch.cuda.synchronize()

    def composed(self):
        """The caller's own forwarding on the other entry points, with vectorised host work."""
        rx_open_wire_batch_device(self.eng, self.alg, self.dw, self.d_pk, self.arena, self.d_status, self.hint_in)
        st = self.d_status.cpu().numpy()                      # statuses to the host
        el = np.flatnonzero(st == L.STATUS_OK)                # every packet here is Message/Relay with a route
        t = self.route_tun[el]
        order = np.argsort(t, kind="stable")                  # arrival order kept inside each tunnel
        ts = t[order]
        first = np.searchsorted(ts, ts, side="left")
        rank = np.empty(len(el), np.uint64)
        rank[order] = np.arange(len(el), dtype=np.uint64) - first.astype(np.uint64) + np.uint64(1)
        ctr = self.tun_host["message_counter"][t] + rank
        np.add.at(self.tun_host["message_counter"], t, np.uint64(1))
        hdr = headers(self.routes["remote_index"][el], ctr)
        desc = relay_desc(self.off[el], ctr, self.out_kid[t])
        m = len(el)
        self.d_hdr[:m].copy_(self.torch.from_numpy(hdr), non_blocking=False)   # upload
        self.d_desc[:m * L.DESC_DTYPE.itemsize].copy_(self.torch.from_numpy(desc.view(np.uint8)))
        self.rows[self.torch.from_numpy(el).to(self.dev), :16] = self.d_hdr[:m]
        L.check(L.lib().neb_seal_batch(self.eng.handle, self.alg, C.c_void_p(self.d_desc.data_ptr()), m,
                                       C.c_void_p(self.arena.data_ptr()), C.c_void_p(self.d_sub.data_ptr()),
                                       self.hint_out, self.stream()), "neb_seal_batch")
        self.torch.cuda.synchronize()

    def check_forms_agree(self):
        self.prepare()
        before = self.arena.clone()
        self.one_call()
        assert bool((self.d_status == 0).all()) and bool((self.d_fwd == 0).all()), "one call: not all forwarded"
        a = self.arena.clone()
        tun_a = self.d_tun.cpu().numpy().view(TX_TUNNEL_DTYPE)["message_counter"].copy()
        self.arena.copy_(before)
        for k in self.in_kid:  # the same window state again
            self.dw.load(int(k), Bits(8192))
        self.composed()
        assert bool((self.d_status == 0).all()) and bool((self.d_sub[:self.n] == 0).all())
        assert bool(self.torch.equal(a, self.arena)), "one call and composed form differ"
        assert np.array_equal(tun_a, self.tun_host["message_counter"])

    def close(self):
        self.dw.destroy()
        for c in self.ciphers:
            L.lib().neb_cipher_destroy(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--keys", default="1,4096")
    ap.add_argument("--alg", choices=["aesgcm", "chachapoly"], default="aesgcm")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forms", choices=["both", "call"], default="both")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("relay_forward_bench: no GPU (this tool measures on the device only)")
    alg = L.ALG_AESGCM if a.alg == "aesgcm" else L.ALG_CHACHAPOLY
    lines = []
    with Engine(0, 2 * max(int(k) for k in a.keys.split(",")) + 64) as eng:
        for nkeys in [int(k) for k in a.keys.split(",")]:
            case = Case(eng, alg, a.n, nkeys)
            try:
                forms = {"one_call": case.one_call}
                if a.forms == "both":
                    case.check_forms_agree()
                    forms["composed"] = case.composed
                times = {f: [] for f in forms}
                for s in range(a.warmup + a.steps):
                    for f, fn in forms.items():
                        case.prepare()
                        t0 = time.perf_counter()
                        fn()
                        dt = time.perf_counter() - t0
                        if s >= a.warmup:
                            times[f].append(dt)
                for f, ts in times.items():
                    med = statistics.median(ts)
                    lines.append({
                        "tool": "relay_forward_bench", "form": f, "alg": a.alg, "packets": a.n, "keys_in": nkeys,
                        "tunnels_out": nkeys, "ad_bytes": AD, "wire_bytes": WIRE, "steps": len(ts),
                        "median_us": round(med * 1e6, 1), "min_us": round(min(ts) * 1e6, 1),
                        "max_us": round(max(ts) * 1e6, 1),
                        "wire_GiBps_median": round(a.n * WIRE / med / 2 ** 30, 1),
                        "device": torch.cuda.get_device_name(0), "build": L.lib().neb_build_id().decode(),
                    })
                    print(json.dumps(lines[-1]), flush=True)
            finally:
                case.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
