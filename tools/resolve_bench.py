"""What the receive resolve (neb_rx_resolve_batch) costs on a device-resident batch, beside the
calls it runs in front of.

Workload: --n wire packets (default 64 Ki) of 1364 bytes in slots of 1408. Shapes, tunnels:relay
indexes in the table: 1:0 and 4096:64. Measures, per algorithm and shape:

  a_resolve          the resolve alone (device events around a run of launches), on direct packets
                     (one probe chain each) and on terminal relay packets (two headers, two chains)
  b_open_wire        neb_rx_open_wire_batch on arrays the caller filled, against
  b_resolve_open     the resolve, then the same call, on arrays it filled: the difference is what the
                     feature costs on the device
  c_plain_from_wire  neb_rx_plain_from_wire on the same batch: the comparator already in the tree, one
                     lane per packet and one header read each
  d_host_form        neb_rx_resolve_batch_host on one thread: CPU time of the GPU box's host, the
                     order of magnitude of the lookups the caller made before
  u_update           neb_index_table_update replacing four live tunnels (others every call), back to back on one
                     stream:
                     wall time of the calling thread per call (the launch through pinned staging,
                     the events), and
  u_rebuild          the same for the calls among them that rebuild the table (they block); only on
                     request (--measures u) and on tables of at least four tunnels

Every figure is the median over windows of at least --window seconds of timed work (device events;
d: a host clock). The two variants of a comparison alternate in one run. The b forms get fresh
counters every step (the packets are re-sealed on the device outside the timed window) so the
replay windows accept them. Before timing, the resolve's arrays must equal the caller-filled ones
and the host form's.

  python tools/resolve_bench.py --out profiles/resolve/bench.jsonl
  rocprofv3 --kernel-trace --stats ... -- python tools/resolve_bench.py --measures a --window 0.05
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
from nebula_amd.hostmap import IndexTable  # noqa: E402
from nebula_amd.noiseutil import Engine  # noqa: E402

WIRE, STRIDE, PAYLOAD = 1364, 1408, 1364 - 32


def headers(subtype, remote_index, counters):
    """header.Encode(1, Message, subtype, remote_index, counter) for arrays -> (n, 16) uint8"""
    h = np.zeros((len(counters), 16), np.uint8)
    h[:, 0], h[:, 1] = 0x11, subtype
    h[:, 4:8] = np.asarray(remote_index, ">u4").reshape(-1, 1).view(np.uint8)
    h[:, 8:16] = np.asarray(counters, ">u8").reshape(-1, 1).view(np.uint8)
    return h


def timed_updates(call, nput, live, slots, window, windows):
    """us of wall time per call of an update that puts nput records over live keys, in `windows`
    windows of at least `window` seconds of calls: ([per small update], [per rebuilding call]). The
    kinds are told apart by the tables' own rule: a call rebuilds when live + tombstones + puts
    pass 3/4 of the slots, and leaves the live records alone. `live`: also what the table holds now."""
    used, small, rebuilt = live, [], []
    for _ in range(windows):
        ns, calls = [0, 0], [0, 0]
        while sum(ns) < window * 1e9 or not calls[1]:
            k = int(used + nput > slots // 4 * 3)
            t0 = time.perf_counter_ns()
            rc = call()
            ns[k] += time.perf_counter_ns() - t0
            calls[k] += 1
            L.check(rc, "update")
            used = live if k else used + nput
        small.append(ns[0] / 1e3 / calls[0])
        rebuilt.append(ns[1] / 1e3 / calls[1])
    return small, rebuilt


class Case:
    def __init__(self, eng, alg, n, ntun, nrelay, seed=1):
        import torch

        self.torch, self.eng, self.alg, self.n, self.ntun, self.nrelay = torch, eng, alg, n, ntun, nrelay
        self.dev = torch.device("cuda", eng.device)
        rng = np.random.default_rng(seed)
        keys = rng.integers(0, 256, (ntun, 32), dtype=np.uint8)
        out = (C.c_void_p * ntun)()
        L.check(L.lib().neb_cipher_create_batch(eng.handle, alg, keys.ctypes.data_as(C.c_void_p), ntun, out),
                "neb_cipher_create_batch")
        self.ciphers = [C.c_void_p(h) for h in out]
        self.kid = np.array([L.lib().neb_cipher_key_id(c) for c in self.ciphers], np.uint32)
        i = np.arange(n)
        self.tt = (i % ntun).astype(np.uint32)  # interleaved tunnels
        self.place, self.per = (i // ntun).astype(np.uint64), -(-n // ntun)
        self.off = (i * STRIDE).astype(np.uint64)
        self.hint = int(self.kid[0]) if ntun == 1 else L.KEYS_MIXED
        self.tindex = rng.permutation(1 << 20)[:ntun].astype(np.uint32) + np.uint32(0x20000000)  # local indexes
        self.rindex = rng.permutation(1 << 20)[:max(nrelay, 1)].astype(np.uint32) + np.uint32(0x40000000)
        self.table = IndexTable(eng, ntun + nrelay)
        rows = np.zeros(ntun + nrelay, L.INDEX_ENTRY_DTYPE)
        rows["index"][:ntun], rows["space"][:ntun], rows["key_id"][:ntun] = self.tindex, L.INDEX_TUNNEL, self.kid
        rows["index"][ntun:], rows["space"][ntun:] = self.rindex[:nrelay], L.INDEX_RELAY
        rows["key_id"][ntun:], rows["flags"][ntun:] = self.kid[np.arange(nrelay) % ntun], L.VIA_TERMINAL
        rows["tunnel"] = L.RELAY_NONE
        self.table.update([], rows)
        self.entries = rows
        self.h_arena = rng.integers(0, 256, n * STRIDE, dtype=np.uint8)
        self.arena = torch.from_numpy(self.h_arena).to(self.dev)
        self.rows = self.arena.view(n, STRIDE)
        pk = np.zeros(n, L.RX_PACKET_DTYPE)
        pk["off"], pk["len"], pk["key_id"] = self.off, WIRE, self.kid[self.tt]
        self.pk = pk
        blank = pk.copy()
        blank["key_id"] = L.KEYS_MIXED
        self.d_pk, self.d_blank = self.up(pk), self.up(blank)
        self.d_route = torch.zeros(n * 8, dtype=torch.uint8, device=self.dev)
        self.d_via = torch.zeros(n * 8, dtype=torch.uint8, device=self.dev)
        self.d_status = torch.zeros(n, dtype=torch.int32, device=self.dev)
        self.d_sub = torch.zeros(n, dtype=torch.int32, device=self.dev)
        self.d_plain = torch.zeros(n * L.PLAIN_PACKET_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        self.d_epoch = torch.ones(int(self.kid.max()) + 1, dtype=torch.int64, device=self.dev)
        self.dw = DeviceWindows(eng, eng.max_keys, 8192)
        w = Bits(8192)
        for k in self.kid:
            self.dw.load(int(k), w)
        self.step = 0

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev)

    def prepare(self):
        """Untimed: this step's datagrams, direct messages sealed in place with fresh counters."""
        self.step += 1
        c = np.uint64(self.step * self.per) + self.place + np.uint64(1)
        self.rows[:, :16] = self.up(headers(0, self.tindex[self.tt], c)).view(self.n, 16)
        d = np.zeros(self.n, L.DESC_DTYPE)
        d["aad_off"], d["aad_len"] = self.off, 16
        d["src_off"] = d["dst_off"] = self.off + np.uint64(16)
        d["len"], d["counter"], d["key_id"] = PAYLOAD, c, self.kid[self.tt]
        dd = self.up(d)
        s = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        L.check(L.lib().neb_seal_batch(self.eng.handle, self.alg, C.c_void_p(dd.data_ptr()), self.n,
                                       C.c_void_p(self.arena.data_ptr()), C.c_void_p(self.d_sub.data_ptr()), self.hint, s),
                "neb_seal_batch")
        self.torch.cuda.synchronize()

    def relay_mix(self):
        """Terminal relay packets: an outer Message/Relay header, the inner header behind it."""
        if not self.nrelay:
            return False
        zeros = np.zeros(self.n, np.uint64)
        self.rows[:, :16] = self.up(headers(1, self.rindex[np.arange(self.n) % self.nrelay], zeros)).view(self.n, 16)
        self.rows[:, 16:32] = self.up(headers(0, self.tindex[self.tt], zeros)).view(self.n, 16)
        self.torch.cuda.synchronize()
        return True

    def resolve(self):
        self.table.resolve_device(self.d_blank, self.arena, None, self.d_route, self.d_via)

    def open_wire(self, d_pk):
        rx_open_wire_batch_device(self.eng, self.alg, self.dw, d_pk, self.arena, self.d_status, self.hint)

    def bare_calls(self):
        """The two enqueue-only calls with their arguments built once: the timed runs then pay the
        C call and the launch, not the Python wrapper."""
        lib, p = L.lib(), lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        s = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        ra = (self.eng.handle, self.table.handle, p(self.d_blank), None, self.n, p(self.arena), p(self.d_route), p(self.d_via), s)
        pa = (self.eng.handle, p(self.d_pk), p(self.d_status), p(self.d_epoch), self.d_epoch.numel(), self.n, p(self.arena),
              p(self.d_plain), s)
        L.check(lib.neb_rx_resolve_batch(*ra), "neb_rx_resolve_batch")
        L.check(lib.neb_rx_plain_from_wire(*pa), "neb_rx_plain_from_wire")
        return (lambda: lib.neb_rx_resolve_batch(*ra)), (lambda: lib.neb_rx_plain_from_wire(*pa))

    def bare_update(self):
        """neb_index_table_update putting four tunnels' own records again, four others every call."""
        groups = [self.entries[k:k + 4].copy() for k in range(0, self.ntun - 3, 4)]
        s = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        args = [(self.table.handle, None, 0, g.ctypes.data_as(C.c_void_p), 4, s) for g in groups]
        turn = iter(range(1 << 62))
        return lambda: L.lib().neb_index_table_update(*args[next(turn) % len(args)])

    def check(self):
        """The device resolve, the caller's arrays and the host form agree; the batch opens."""
        self.prepare()
        self.resolve()
        self.open_wire(self.d_blank)
        self.torch.cuda.synchronize()
        assert bool((self.d_status == 0).all()), "a packet did not open on the resolved arrays"
        got = self.d_blank.cpu().numpy().view(L.RX_PACKET_DTYPE)
        assert got.tobytes() == self.pk.tobytes(), "the resolve's key_ids differ from the caller's"
        host = self.pk.copy()
        host["key_id"] = 0
        self.h_arena = self.arena.cpu().numpy()
        self.table.resolve_host(host, self.h_arena)
        assert host.tobytes() == self.pk.tobytes(), "the host form differs"

    def timed_launches(self, fn, window):
        """us per call of an enqueue-only call: device events around a run long enough for the window."""
        t = self.torch
        for _ in range(20):
            fn()
        t.cuda.synchronize()
        count, us = 200, None
        while True:
            a, b = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(count):
                fn()
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            us = ms * 1e3 / count
            if ms >= window * 1e3:
                return us, count
            count = int(count * max(2.0, 1.2 * window * 1e3 / max(ms, 1e-3)))

    def close(self):
        self.table.close()
        self.dw.destroy()
        for c in self.ciphers:
            L.lib().neb_cipher_destroy(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--shapes", default="1:0,4096:64", help="tunnels:relay indexes, comma separated")
    ap.add_argument("--algs", default="aesgcm,chachapoly")
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed work per window, at least")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--measures", default="a,b,c,d")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("resolve_bench: no GPU (this tool measures on the device only)")
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    measures = a.measures.split(",")
    lines = []

    def emit(case, alg_name, measure, mix, windows_us, **more):
        lines.append({"tool": "resolve_bench", "measure": measure, "mix": mix, "alg": alg_name, "packets": case.n,
                      "tunnels": case.ntun, "relay_indexes": case.nrelay, "wire_bytes": WIRE,
                      "median_us": round(statistics.median(windows_us), 2), "windows_us": [round(x, 2) for x in windows_us],
                      "window_s": a.window, "device": torch.cuda.get_device_name(0),
                      "build": L.lib().neb_build_id().decode(), **more})
        print(json.dumps(lines[-1]), flush=True)

    with Engine(0, max(t for t, _ in shapes) + 64) as eng:
        for alg_name in a.algs.split(","):
            alg = L.ALG_AESGCM if alg_name == "aesgcm" else L.ALG_CHACHAPOLY
            for ntun, nrelay in shapes:
                case = Case(eng, alg, a.n, ntun, nrelay)
                try:
                    case.check()
                    if "b" in measures:  # alternating, step by step, until each form has its windows
                        forms = {"b_open_wire": lambda: case.open_wire(case.d_pk),
                                 "b_resolve_open": lambda: (case.resolve(), case.open_wire(case.d_blank))}
                        done = {f: [] for f in forms}
                        acc = {f: [0.0, 0] for f in forms}
                        warm = 3
                        while any(len(v) < a.windows for v in done.values()):
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
                            emit(case, alg_name, f, "direct", v[:a.windows])
                    case.prepare()
                    case.open_wire(case.d_pk)  # statuses of an opened batch, for c
                    torch.cuda.synchronize()
                    resolve, plain = case.bare_calls()
                    mixes = [("direct", lambda: True), ("terminal_relay", case.relay_mix)]
                    for mix, setup in mixes:
                        if not setup():
                            continue
                        ra, rc = [], []
                        for _ in range(a.windows):  # a and c alternate, window by window
                            if "a" in measures:
                                ra.append(case.timed_launches(resolve, a.window))
                            if "c" in measures and mix == "direct":
                                rc.append(case.timed_launches(plain, a.window))
                        if ra:
                            emit(case, alg_name, "a_resolve", mix, [u for u, _ in ra], launches_per_window=ra[-1][1])
                        if rc:
                            emit(case, alg_name, "c_plain_from_wire", mix, [u for u, _ in rc], launches_per_window=rc[-1][1])
                        if "d" in measures:
                            h_arena = case.arena.cpu().numpy()
                            host = case.pk.copy()
                            ws = []
                            for _ in range(a.windows):
                                t0, calls = time.perf_counter(), 0
                                while time.perf_counter() - t0 < a.window:
                                    case.table.resolve_host(host, h_arena)
                                    calls += 1
                                ws.append((time.perf_counter() - t0) * 1e6 / calls)
                            emit(case, alg_name, "d_host_form", mix, ws, clock="CPU time of the GPU box's host, one thread")
                    if "u" in measures and ntun >= 4:  # last: it leaves tombstones behind
                        live = ntun + nrelay
                        small, rebuilt = timed_updates(case.bare_update(), 4, live, max(16, 1 << (4 * live - 1).bit_length()),
                                                       a.window, a.windows)
                        torch.cuda.synchronize()
                        emit(case, alg_name, "u_update", "replace_4", small, clock="wall time of the calling thread")
                        emit(case, alg_name, "u_rebuild", "replace_4", rebuilt, clock="wall time of the calling thread")
                        case.check()  # the table still resolves as before
                finally:
                    case.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
