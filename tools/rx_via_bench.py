"""Receiving through relays on a device-resident batch: neb_rx_open_via_batch (one call) against the
same work composed by a caller from neb_rx_open_wire_batch (receive, statuses to the host, a second
neb_rx_packet array built on the CPU and uploaded, receive again), and against one plain
neb_rx_open_wire_batch of direct packets that carry the same payload bytes (the yardstick: what the
node would pay if it were reached directly) and one of the relay packets alone (VerifyRelay through
the windows: phase 1 by itself).

Workload: --n terminal relay packets (default 64 Ki) of 1364 wire bytes: outer header 16, an inner
wire packet of 1332 (16 + 1300 + 16), outer tag 16. Shapes: 1 relay -> 1 peer behind it, and
64 relays -> 4096 peers. Every step gets fresh outer and inner counters (the packets are re-sealed
on the device, outside the timed window) so the windows accept them. The forms are timed in one
process, alternating, with a host clock around work that ends in a device synchronize; GiB/s of
wire bytes from the median. Before timing, the one call and the composed form run on the same input
and must leave the same bytes and statuses.

  python tools/rx_via_bench.py --out profiles/rx_via/bench.jsonl
  rocprofv3 --kernel-trace --stats ... -- python tools/rx_via_bench.py --forms call --steps 5
  ... --forms call --terminal none   (no relayed traffic: phase 2 must not launch anything)
  ... --terminal eighth              (one packet in eight is relayed: phase 2 over a sparse batch)
  ... --forms plain                  (the launches of the plain receive, to compare)
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
from nebula_amd.noiseutil import Engine  # noqa: E402
from nebula_amd.relay import rx_open_via_batch_device  # noqa: E402

PAYLOAD, INNER, WIRE, STRIDE = 1300, 1332, 1364, 1408
DSTRIDE = 1344  # the direct yardstick's slots: one 1332-byte wire packet each


def headers(subtype, remote_index, counters):
    """header.Encode(1, Message, subtype, remote_index, counter) for arrays -> (n, 16) uint8"""
    h = np.zeros((len(counters), 16), np.uint8)
    h[:, 0], h[:, 1] = 0x11, subtype
    h[:, 4:8] = np.asarray(remote_index, ">u4").reshape(-1, 1).view(np.uint8)
    h[:, 8:16] = np.asarray(counters, ">u8").reshape(-1, 1).view(np.uint8)
    return h


def desc(aad_off, aad_len, data_off, data_len, counters, key_ids):
    d = np.zeros(len(counters), L.DESC_DTYPE)
    d["aad_off"], d["aad_len"] = aad_off, aad_len
    d["src_off"] = d["dst_off"] = data_off
    d["len"], d["counter"], d["key_id"] = data_len, counters, key_ids
    return d


class Case:
    def __init__(self, eng, alg, n, nrelay, ntarget, terminal="all", seed=1):
        import torch

        self.torch, self.eng, self.alg, self.n = torch, eng, alg, n
        self.dev = torch.device("cuda", eng.device)
        rng = np.random.default_rng(seed)
        nk = nrelay + ntarget
        keys = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
        out = (C.c_void_p * nk)()
        L.check(L.lib().neb_cipher_create_batch(eng.handle, alg, keys.ctypes.data_as(C.c_void_p), nk, out),
                "neb_cipher_create_batch")
        self.ciphers = [C.c_void_p(h) for h in out]
        kid = np.array([L.lib().neb_cipher_key_id(c) for c in self.ciphers], np.uint32)
        self.relay_kid, self.target_kid = kid[:nrelay], kid[nrelay:]
        i = np.arange(n)
        self.rt, self.tt = (i % nrelay).astype(np.uint32), (i % ntarget).astype(np.uint32)  # interleaved tunnels
        self.rplace, self.tplace = (i // nrelay).astype(np.uint64), (i // ntarget).astype(np.uint64)
        self.rper, self.tper = -(-n // nrelay), -(-n // ntarget)
        self.off, self.doff = (i * STRIDE).astype(np.uint64), (i * DSTRIDE).astype(np.uint64)
        self.hint = int(self.relay_kid[0]) if nrelay == 1 else L.KEYS_MIXED
        self.inner_hint = int(self.target_kid[0]) if ntarget == 1 else L.KEYS_MIXED
        self.arena = torch.from_numpy(rng.integers(0, 256, n * STRIDE, dtype=np.uint8)).to(self.dev)
        self.rows = self.arena.view(n, STRIDE)
        self.darena = torch.zeros(n * DSTRIDE, dtype=torch.uint8, device=self.dev)
        self.drows = self.darena.view(n, DSTRIDE)
        self.drows[:, 16:16 + PAYLOAD] = self.rows[:, 32:32 + PAYLOAD]  # the same payload bytes
        pk = np.zeros(n, L.RX_PACKET_DTYPE)
        pk["off"], pk["len"], pk["key_id"] = self.off, WIRE, self.relay_kid[self.rt]
        via = np.zeros(n, L.RX_VIA_DTYPE)
        via["key_id"] = self.target_kid[self.tt]
        via["flags"] = {"all": L.VIA_TERMINAL, "none": 0, "eighth": np.where(i % 8 == 0, L.VIA_TERMINAL, 0)}[terminal]
        self.via = via
        dpk = np.zeros(n, L.RX_PACKET_DTYPE)
        dpk["off"], dpk["len"], dpk["key_id"] = self.doff, INNER, self.target_kid[self.tt]
        self.d_pk, self.d_via, self.d_dpk = self.up(pk), self.up(via), self.up(dpk)
        i32 = lambda: torch.zeros(n, dtype=torch.int32, device=self.dev)  # noqa: E731
        self.d_status, self.d_ist, self.d_sub, self.d_dstatus = i32(), i32(), i32(), i32()
        self.d_inner = torch.zeros(n * L.RX_PACKET_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        self.d_inner2 = torch.zeros(n * L.RX_PACKET_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        self.dw, self.ddw = DeviceWindows(eng, eng.max_keys, 8192), DeviceWindows(eng, eng.max_keys, 8192)
        self.fresh_windows()
        self.step = 0

    def fresh_windows(self):
        w = Bits(8192)
        for k in np.concatenate([self.relay_kid, self.target_kid]):
            self.dw.load(int(k), w)
        for k in self.target_kid:
            self.ddw.load(int(k), w)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to(self.dev)

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def seal(self, d, arena, hint):
        dd = self.up(d)
        L.check(L.lib().neb_seal_batch(self.eng.handle, self.alg, C.c_void_p(dd.data_ptr()), self.n,
                                       C.c_void_p(arena.data_ptr()), C.c_void_p(self.d_sub.data_ptr()), hint,
                                       self.stream()), "neb_seal_batch")
        self.torch.cuda.synchronize()

    def counters(self):
        self.step += 1
        return (np.uint64(self.step * self.rper) + self.rplace + np.uint64(1),
                np.uint64(self.step * self.tper) + self.tplace + np.uint64(1))

    def prepare_via(self):
        """Untimed: this step's datagrams. The inner packets are sealed in place under the peers'
        keys with fresh counters, then wrapped: a fresh outer header and the relay's AD-only tag."""
        rc, tc = self.counters()
        self.rows[:, 16:32] = self.up(headers(0, 0x2000 + self.tt, tc)).view(self.n, 16)
        self.seal(desc(self.off + np.uint64(16), 16, self.off + np.uint64(32), PAYLOAD, tc, self.target_kid[self.tt]),
                  self.arena, self.inner_hint)
        self.rows[:, :16] = self.up(headers(1, 0x1000 + self.rt, rc)).view(self.n, 16)
        self.seal(desc(self.off, 16 + INNER, self.off + np.uint64(16 + INNER), 0, rc, self.relay_kid[self.rt]),
                  self.arena, self.hint)

    def prepare_plain(self):
        _, tc = self.counters()
        self.drows[:, :16] = self.up(headers(0, 0x2000 + self.tt, tc)).view(self.n, 16)
        self.seal(desc(self.doff, 16, self.doff + np.uint64(16), PAYLOAD, tc, self.target_kid[self.tt]), self.darena,
                  self.inner_hint)

    def one_call(self):
        rx_open_via_batch_device(self.eng, self.alg, self.dw, self.d_pk, self.d_via, self.arena, self.d_status,
                                 self.d_inner, self.d_ist, self.hint, self.inner_hint)
        self.torch.cuda.synchronize()

    def composed(self):
        """The caller's own two-level receive on neb_rx_open_wire_batch, with vectorised host work;
        the second batch holds the inner packets only, in arrival order."""
        rx_open_wire_batch_device(self.eng, self.alg, self.dw, self.d_pk, self.arena, self.d_status, self.hint)
        st = self.d_status.cpu().numpy()                                  # statuses to the host
        el = np.flatnonzero((st == L.STATUS_OK) & ((self.via["flags"] & L.VIA_TERMINAL) != 0))  # all Message/Relay here
        self.el = el
        m = len(el)
        if m:
            inner = np.zeros(m, L.RX_PACKET_DTYPE)                        # the second array, on the CPU
            inner["off"], inner["len"], inner["key_id"] = self.off[el] + np.uint64(16), WIRE - 32, self.via["key_id"][el]
            d_in = self.d_inner2[:m * 16]
            d_in.copy_(self.torch.from_numpy(inner.view(np.uint8)))       # upload
            rx_open_wire_batch_device(self.eng, self.alg, self.dw, d_in, self.arena, self.d_ist[:m], self.inner_hint)
        self.torch.cuda.synchronize()

    def relay_verify(self):
        """Phase 1 alone: the plain wire receive of the relay packets (VerifyRelay through the windows)."""
        rx_open_wire_batch_device(self.eng, self.alg, self.dw, self.d_pk, self.arena, self.d_status, self.hint)
        self.torch.cuda.synchronize()

    def plain(self):
        rx_open_wire_batch_device(self.eng, self.alg, self.ddw, self.d_dpk, self.darena, self.d_dstatus, self.inner_hint)
        self.torch.cuda.synchronize()

    def check_forms_agree(self):
        self.prepare_via()
        before = self.arena.clone()
        self.one_call()
        assert bool((self.d_status == 0).all()), "one call: an outer packet did not verify"
        a, ist_a = self.arena.clone(), self.d_ist.cpu().numpy()
        want = np.where(self.via["flags"] != 0, L.STATUS_OK, L.STATUS_NOT_RELAYED)
        assert np.array_equal(ist_a, want), "one call: an inner packet did not open"
        self.arena.copy_(before)
        self.fresh_windows()  # the same window state again
        self.composed()
        assert bool((self.d_status == 0).all())
        ist_b = np.full(self.n, L.STATUS_NOT_RELAYED, np.int32)
        ist_b[self.el] = self.d_ist[:len(self.el)].cpu().numpy()
        assert np.array_equal(ist_a, ist_b), "one call and composed form: statuses differ"
        assert bool(self.torch.equal(a, self.arena)), "one call and composed form: bytes differ"
        if bool(want.min() == want.max() == 0):  # all opened: the direct packets' payload, byte for byte
            assert bool(self.torch.equal(self.rows[:, 32:32 + PAYLOAD], self.drows[:, 16:16 + PAYLOAD]))

    def close(self):
        self.dw.destroy()
        self.ddw.destroy()
        for c in self.ciphers:
            L.lib().neb_cipher_destroy(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--shapes", default="1:1,64:4096", help="relays:peers, comma separated")
    ap.add_argument("--algs", default="aesgcm,chachapoly")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forms", choices=["all", "call", "plain"], default="all")
    ap.add_argument("--terminal", choices=["all", "none", "eighth"], default="all",
                    help="none: no via record is terminal (a batch without relayed traffic); eighth: every 8th is")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("rx_via_bench: no GPU (this tool measures on the device only)")
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    lines = []
    with Engine(0, max(r + t for r, t in shapes) + 64) as eng:
        for alg_name in a.algs.split(","):
            alg = L.ALG_AESGCM if alg_name == "aesgcm" else L.ALG_CHACHAPOLY
            for nrelay, ntarget in shapes:
                case = Case(eng, alg, a.n, nrelay, ntarget, a.terminal)
                try:
                    forms = {}
                    if a.forms in ("all", "call"):
                        forms["one_call"] = (case.prepare_via, case.one_call)
                    if a.forms == "all":
                        case.check_forms_agree()
                        forms["composed"] = (case.prepare_via, case.composed)
                        forms["relay_verify"] = (case.prepare_via, case.relay_verify)
                    if a.forms in ("all", "plain"):
                        forms["plain_direct"] = (case.prepare_plain, case.plain)
                    times = {f: [] for f in forms}
                    for s in range(a.warmup + a.steps):
                        for f, (prep, fn) in forms.items():
                            prep()
                            t0 = time.perf_counter()
                            fn()
                            dt = time.perf_counter() - t0
                            if s >= a.warmup:
                                times[f].append(dt)
                    for f, ts in times.items():
                        med = statistics.median(ts)
                        wire = INNER if f == "plain_direct" else WIRE
                        lines.append({
                            "tool": "rx_via_bench", "form": f, "alg": alg_name, "packets": a.n, "relays": nrelay,
                            "peers": ntarget, "terminal": a.terminal, "wire_bytes": wire, "payload_bytes": PAYLOAD,
                            "steps": len(ts), "median_us": round(med * 1e6, 1), "min_us": round(min(ts) * 1e6, 1),
                            "max_us": round(max(ts) * 1e6, 1), "wire_GiBps_median": round(a.n * wire / med / 2 ** 30, 1),
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
