"""The TX batch through relays on a device-resident batch of TUN reads: neb_tx_seal_via_batch (one
call) against (a) neb_tx_seal_batch of the same reads, the direct cost, and (b) the same via wires
composed by a caller from the other entry points (direct TX, the wires to the host, every packet
moved 16 bytes and the Message/Relay headers and relay counters written in numpy, upload, AD-only
neb_seal_batch).

Workload: --reads IPv4/TCP TSO superpackets of 45 x 1448 B (default 1456: 65 520 wires, no partial
pass of the single-key seal; DESIGN §3.5's shape), AES-256-GCM. Two cases: every read to one target
through one relay (key_hint = the target's key, both seals single-key), and 4096 targets through
64 relays (both seals mixed-key). The forms are timed in one process, alternating, each between two
HIP events on the stream (the composed form's host work lies between its events); the median of
--steps calls after --warmup. Before timing, the one call and the composed form run from the same
counters and must leave the same wires.

  python tools/tx_via_bench.py --out profiles/tx_via/bench.jsonl
  rocprofv3 --kernel-trace --stats ... -- python tools/tx_via_bench.py --forms call --cases 1:1 --steps 5
  (and --forms direct for the direct batch's kernels beside them)
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
from bench import tso_superpackets  # noqa: E402
from nebula_amd import _lib as L  # noqa: E402
from nebula_amd.inside import (TX_PACKET_DTYPE, TX_TUNNEL_DTYPE, DeviceTxBatch, slot_bytes,  # noqa: E402
                               slot_bytes_via)
from nebula_amd.noiseutil import Engine  # noqa: E402

MSS, PER = 1448, 45
SEG = 40 + MSS                    # one segment: IPv4 + TCP headers + MSS
DIRECT, VIA = SEG + 32, SEG + 64  # wire bytes


class Case:
    def __init__(self, eng, nreads, ntargets, nrelays, seed=1):
        import torch

        self.torch, self.eng, self.alg = torch, eng, L.ALG_AESGCM
        self.dev = torch.device("cuda", eng.device)
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
        self.tun0 = np.zeros(nt, TX_TUNNEL_DTYPE)
        self.tun0["message_counter"] = 2 + 1000 * np.arange(nt)
        self.tun0["key_id"], self.tun0["remote_index"] = kid, 0x9000 + np.arange(nt)
        self.via = np.zeros(nt, L.RELAY_ROUTE_DTYPE)
        self.via["tunnel"] = L.RELAY_NONE
        self.via["tunnel"][nrelays:] = np.arange(ntargets) % nrelays
        self.via["remote_index"][nrelays:] = 0x7000 + np.arange(ntargets)
        arena, nsp, size, stride, per = tso_superpackets(PER * nreads, MSS)
        assert nsp == nreads and per == PER
        self.nreads, self.nw, self.tun_bytes = nsp, nsp * per, nsp * size
        pk = np.zeros(nsp, TX_PACKET_DTYPE)
        self.read_tun = (nrelays + (np.arange(nsp) * 7 + 3) % ntargets).astype(np.uint32)
        for i in range(nsp):
            pk[i] = (i * stride, size, self.read_tun[i], 1, 1, 40, MSS, 20, 16, 0)
        self.hint = int(kid[nrelays]) if ntargets == 1 else L.KEYS_MIXED
        self.hint_relay = int(kid[0]) if nrelays == 1 else L.KEYS_MIXED
        assert slot_bytes(SEG) == DIRECT and slot_bytes_via(SEG) == VIA
        self.direct = DeviceTxBatch(eng, self.alg, self.tun0, pk, arena, self.nw * DIRECT, self.nw, self.hint)
        self.one = DeviceTxBatch(eng, self.alg, self.tun0, pk, arena, self.nw * VIA, self.nw, self.hint, via=self.via)
        # the composed form's own buffers: the via wires, their descriptors and statuses
        self.c_out = torch.zeros(self.nw * VIA, dtype=torch.uint8, device=self.dev)
        self.c_desc = torch.zeros(self.nw * L.DESC_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        self.c_status = torch.zeros(self.nw, dtype=torch.int32, device=self.dev)
        self.c_host = np.zeros((self.nw, VIA), np.uint8)
        self.relay_ctr = self.tun0["message_counter"][:nrelays].copy()  # kept on the host by this form
        self.wire_relay = np.repeat(self.via["tunnel"][self.read_tun], PER)  # each wire's relay tunnel
        self.wire_ri = np.repeat(self.via["remote_index"][self.read_tun], PER)

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def reset(self):
        self.direct.reset_counters()
        self.one.reset_counters()
        self.relay_ctr = self.tun0["message_counter"][:self.nrelays].copy()

    def one_call(self):
        self.one.seal()

    def direct_tx(self):
        self.direct.seal()

    def composed(self):
        """The caller's own SendVia on the other entry points, with vectorised host work."""
        torch = self.torch
        self.direct.seal()
        wires = self.direct.out.cpu().numpy().reshape(self.nw, DIRECT)       # the wires to the host
        t = self.wire_relay
        order = np.argsort(t, kind="stable")                                  # batch order kept inside each relay
        ts = t[order]
        rank = np.empty(self.nw, np.uint64)
        rank[order] = np.arange(self.nw, dtype=np.uint64) - np.searchsorted(ts, ts, side="left").astype(np.uint64)
        ctr = self.relay_ctr[t] + rank + np.uint64(1)
        np.add.at(self.relay_ctr, t, np.uint64(1))
        h = self.c_host
        h[:, 16:16 + DIRECT] = wires                                          # every packet 16 bytes further
        h[:, 0], h[:, 1], h[:, 2:4] = 0x11, 1, 0
        h[:, 4:8] = self.wire_ri.astype(">u4").reshape(-1, 1).view(np.uint8)
        h[:, 8:16] = ctr.astype(">u8").reshape(-1, 1).view(np.uint8)
        d = np.zeros(self.nw, L.DESC_DTYPE)
        off = np.arange(self.nw, dtype=np.uint64) * np.uint64(VIA)
        d["aad_off"], d["aad_len"] = off, VIA - 16
        d["src_off"] = d["dst_off"] = off + np.uint64(VIA - 16)
        d["counter"], d["key_id"] = ctr, self.tun0["key_id"][t]
        self.c_out.copy_(torch.from_numpy(h.reshape(-1)))                     # upload
        self.c_desc.copy_(torch.from_numpy(d.view(np.uint8)))
        L.check(L.lib().neb_seal_batch(self.eng.handle, self.alg, C.c_void_p(self.c_desc.data_ptr()), self.nw,
                                       C.c_void_p(self.c_out.data_ptr()), C.c_void_p(self.c_status.data_ptr()),
                                       self.hint_relay, self.stream()), "neb_seal_batch")

    def check_forms_agree(self):
        torch = self.torch
        self.reset()
        self.one_call()
        torch.cuda.synchronize()
        r = self.one.result()
        assert len(r.wires) == self.nw and (r.wire_status == 0).all() and (r.packet_status == 0).all()
        assert (r.wires["reserved"] == L.TX_WIRE_VIA).all() and (r.wires["len"] == VIA).all()
        self.reset()
        self.composed()
        torch.cuda.synchronize()
        assert bool((self.c_status == 0).all())
        assert bool(torch.equal(self.one.out, self.c_out)), "one call and composed form differ"
        assert np.array_equal(r.tunnels["message_counter"][:self.nrelays], self.relay_ctr)

    def close(self):
        for c in self.ciphers:
            L.lib().neb_cipher_destroy(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1456)
    ap.add_argument("--cases", default="1:1,4096:64", help="targets:relays, comma separated")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forms", choices=["all", "call", "direct"], default="all")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("tx_via_bench: no GPU (this tool measures on the device only)")
    cases = [tuple(int(x) for x in c.split(":")) for c in a.cases.split(",")]
    lines = []
    with Engine(0, max(t + r for t, r in cases) + 64) as eng:
        for ntargets, nrelays in cases:
            case = Case(eng, a.reads, ntargets, nrelays)
            try:
                forms = {"direct_tx": case.direct_tx} if a.forms == "direct" else {"one_call": case.one_call}
                if a.forms == "all":
                    case.check_forms_agree()
                    forms["direct_tx"] = case.direct_tx
                    forms["composed"] = case.composed
                times = {f: [] for f in forms}
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                for s in range(a.warmup + a.steps):
                    for f, fn in forms.items():
                        torch.cuda.synchronize()
                        ev0.record()
                        fn()
                        ev1.record()
                        torch.cuda.synchronize()
                        if s >= a.warmup:
                            times[f].append(ev0.elapsed_time(ev1) * 1e-3)
                med = {f: statistics.median(ts) for f, ts in times.items()}
                for f, ts in times.items():
                    wire = DIRECT if f == "direct_tx" else VIA
                    line = {
                        "tool": "tx_via_bench", "form": f, "alg": "aesgcm", "reads": case.nreads, "wires": case.nw,
                        "targets": ntargets, "relays": nrelays, "wire_bytes": wire, "steps": len(ts),
                        "median_us": round(med[f] * 1e6, 1), "min_us": round(min(ts) * 1e6, 1),
                        "max_us": round(max(ts) * 1e6, 1),
                        "tun_GiBps_median": round(case.tun_bytes / med[f] / 2 ** 30, 1),
                        "wire_GiBps_median": round(case.nw * wire / med[f] / 2 ** 30, 1),
                        "device": torch.cuda.get_device_name(0), "build": L.lib().neb_build_id().decode(),
                    }
                    if f == "one_call" and "direct_tx" in med:
                        line["x_direct_tx"] = round(med[f] / med["direct_tx"], 3)
                        line["x_composed"] = round(med[f] / med["composed"], 3)
                    lines.append(line)
                    print(json.dumps(line), flush=True)
            finally:
                case.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
