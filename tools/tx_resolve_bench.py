"""What the TX resolve (neb_tx_resolve_batch) costs on a device-resident batch of TUN reads, beside
the seal it runs in front of and the receive resolve, the closest kernel already in the tree.

Workloads: --plain plain IPv4/UDP reads of 1300 bytes (default 64 Ki), each 2 bytes past a 16-byte
boundary as behind a virtio header, and --tso IPv4/TCP TSO reads of 45 x 1448 B (default 1456).
Tables, hosts:routes: 1:0 and 4096:64 (routes of three prefix lengths, four gateways each, the own
network a /8). Destination mixes: in_network (every read names a host entry) and routed (every read
falls to a route and its ECMP bucket; the gateway's host entry gives the tunnel). Measures:

  a_tx_resolve_fw    the resolve alone with the 48-byte neb_fw_packet store, per call
  a_tx_resolve       the same without it (tunnel and status only)
  a_rx_resolve       neb_rx_resolve_batch per call at the same packet count, in the same run
  b_seal             neb_tx_seal_batch on tunnels the caller filled, against
  b_resolve_seal     the resolve, then the same seal on the tunnels it wrote, on one stream
  c_host_form        neb_tx_resolve_batch_host on one thread of this box's CPU, on the same batch, into
                     output arrays allocated once (wall time per call)
  u_update, u_rebuild  neb_tx_table_update_hosts replacing four live hosts (others every call), back to back on one
                     stream:
                     wall time of the calling thread per call, and per call that rebuilds (as
                     tools/resolve_bench.py); only on request (--measures u), plain in_network reads,
                     tables of at least four hosts

Every figure is the median over windows of at least --window seconds of timed work (device events;
c: a host clock). The variants of a comparison alternate in one run. Before timing, the device
resolve must equal the caller-filled tunnels and the host form.

  python tools/tx_resolve_bench.py --out profiles/tx_resolve/bench.jsonl
  rocprofv3 --kernel-trace --stats ... -- python tools/tx_resolve_bench.py --measures a --window 0.05
"""
import argparse
import ctypes as C
import ipaddress
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
from nebula_amd.hostmap import IndexTable, TxTable, tx_hosts, tx_routes  # noqa: E402
from nebula_amd.inside import TX_PACKET_DTYPE, TX_TUNNEL_DTYPE, DeviceTxBatch, slot_bytes  # noqa: E402
from nebula_amd.noiseutil import Engine  # noqa: E402
from resolve_bench import timed_updates  # noqa: E402

MSS, PER, PLAIN = 1448, 45, 1300


def be32(a):
    return np.asarray(a, ">u4").reshape(-1, 1).view(np.uint8)


class Case:
    def __init__(self, eng, kind, n, nhosts, nroutes, mix, seed=1):
        import torch

        self.torch, self.eng, self.alg, self.kind, self.n, self.mix = torch, eng, L.ALG_AESGCM, kind, n, mix
        self.nhosts, self.nroutes = nhosts, nroutes
        self.dev = torch.device("cuda", eng.device)
        rng = np.random.default_rng(seed)
        keys = rng.integers(0, 256, (nhosts, 32), dtype=np.uint8)
        out = (C.c_void_p * nhosts)()
        L.check(L.lib().neb_cipher_create_batch(eng.handle, self.alg, keys.ctypes.data_as(C.c_void_p), nhosts, out),
                "neb_cipher_create_batch")
        self.ciphers = [C.c_void_p(h) for h in out]
        kid = np.array([L.lib().neb_cipher_key_id(c) for c in self.ciphers], np.uint32)
        tun = np.zeros(nhosts, TX_TUNNEL_DTYPE)
        tun["message_counter"], tun["key_id"], tun["remote_index"] = 2 + 1000 * np.arange(nhosts), kid, 0x9000 + np.arange(nhosts)
        # hosts 10.1.x.y in the own network 10.0.0.1/8; host h is tunnel h
        host_ip = (0x0A010000 + np.arange(nhosts)).astype(np.uint32)
        self.table = TxTable(eng, nhosts, max(nroutes, 1), 4 * max(nroutes, 1))
        self.table.set_own(["10.0.0.1/8"], True, True)
        self.table.update_hosts([], tx_hosts([(str(ipaddress.ip_address(int(a))), h) for h, a in enumerate(host_ip)]))
        rows, self.route_net = [], []
        for r in range(nroutes):  # three prefix lengths; four gateways each, weights 1:1:1:1
            net = [f"172.16.{r}.0/24", f"172.{32 + r}.0.0/16", f"{100 + r}.0.0.0/8"][r % 3]
            gws = [int(rng.integers(0, nhosts)) for _ in range(4)]
            rows.append((net, [(str(ipaddress.ip_address(int(host_ip[g]))), 1) for g in gws]))
            self.route_net.append(int(ipaddress.ip_network(net).network_address) + 9)
        self.table.set_routes(tx_routes(rows))
        i = np.arange(n)
        sport, dport = (40000 + i % 20000).astype(np.uint16), (443 + i % 7).astype(np.uint16)
        if mix == "in_network":
            dst = host_ip[(i * 7 + 3) % nhosts]
        else:
            dst = np.array(self.route_net, np.uint32)[i % nroutes]
        if kind == "plain":
            size, stride = PLAIN, 1328  # 16-byte slots, the read 2 bytes in
            arena = rng.integers(0, 256, n * stride + 64, dtype=np.uint8)
            rowsv = arena[:n * stride].reshape(n, stride)[:, 2:]
            hdr = np.zeros(28, np.uint8)
            hdr[0], hdr[2:4], hdr[8], hdr[9] = 0x45, (PLAIN >> 8, PLAIN & 255), 64, 17
            hdr[12:16] = (10, 0, 0, 1)
            rowsv[:, :28] = hdr
            rowsv[:, 16:20], rowsv[:, 20:22], rowsv[:, 22:24] = be32(dst), sport.astype(">u2").reshape(-1, 1).view(np.uint8), \
                dport.astype(">u2").reshape(-1, 1).view(np.uint8)
            off, vnet = i * stride + 2, (0, 0, 0, 0, 0, 0)
            self.nw = n
            out_cap = n * slot_bytes(PLAIN)
        else:
            arena, nsp, size, stride, per = tso_superpackets(PER * n, MSS)
            assert nsp == n and per == PER
            rowsv = arena[:n * stride].reshape(n, stride)
            rowsv[:, 16:20], rowsv[:, 20:22], rowsv[:, 22:24] = be32(dst), sport.astype(">u2").reshape(-1, 1).view(np.uint8), \
                dport.astype(">u2").reshape(-1, 1).view(np.uint8)
            off, vnet = i * stride, (1, 1, 40, MSS, 20, 16)
            self.nw = n * PER
            out_cap = self.nw * slot_bytes(40 + MSS)
        self.h_arena = arena
        pk = np.zeros(n, TX_PACKET_DTYPE)
        pk["in_off"], pk["len"] = off, size
        for f, v in zip(("vnet_flags", "gso_type", "hdr_len", "gso_size", "csum_start", "csum_offset"), vnet):
            pk[f] = v
        # the caller's own lookup, for the filled form: the host form of the same table
        self.pk_filled = pk.copy()
        self.h_fw, self.h_status = self.table.resolve_host(self.pk_filled, arena)
        assert (self.h_status == 0).all(), "a read of the workload does not resolve"
        if mix == "routed":
            assert (self.h_fw["flags"] & L.FW_ROUTED).all()
            assert n < 8 * nroutes or len(set(self.h_fw["gateway"].tolist())) > nroutes  # ECMP spreads the reads
        pk["tunnel"] = L.TX_NO_TUNNEL
        self.pk_blank = pk
        hint = int(kid[0]) if nhosts == 1 else L.KEYS_MIXED
        self.filled = DeviceTxBatch(eng, self.alg, tun, self.pk_filled, arena, out_cap, self.nw, hint)
        self.blank = DeviceTxBatch(eng, self.alg, tun, pk, arena, out_cap, self.nw, hint)
        self.d_fw = torch.zeros(n * L.FW_PACKET_DTYPE.itemsize, dtype=torch.uint8, device=self.dev)
        self.d_status = torch.zeros(n, dtype=torch.int32, device=self.dev)
        # the receive resolve at the same count: n headers naming the tunnels' local indexes
        self.index = IndexTable(eng, nhosts)
        rows = np.zeros(nhosts, L.INDEX_ENTRY_DTYPE)
        rows["index"], rows["key_id"], rows["tunnel"] = 0x20000000 + np.arange(nhosts), kid, L.RELAY_NONE
        self.index.update([], rows)
        h = np.zeros((n, 16), np.uint8)
        h[:, 0] = 0x11
        h[:, 4:8] = be32(0x20000000 + (i * 7 + 3) % nhosts)
        rx = np.zeros(n, L.RX_PACKET_DTYPE)
        rx["off"], rx["len"], rx["key_id"] = i * 16, 16, L.KEYS_MIXED
        self.rx_want = kid[(i * 7 + 3) % nhosts]
        self.d_rx_arena, self.d_rx = self.up(h), self.up(rx)
        self.d_route = torch.zeros(n * 8, dtype=torch.uint8, device=self.dev)
        self.d_via = torch.zeros(n * 8, dtype=torch.uint8, device=self.dev)

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev)

    def resolve_seal(self):
        self.table.resolve_device(self.blank.packets, self.blank.inp, self.d_fw, self.d_status)
        self.blank.seal()

    def bare_calls(self):
        """The enqueue-only calls with their arguments built once: the timed runs then pay the C call
        and the launch, not the Python wrapper."""
        lib, p = L.lib(), lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        s = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        b = self.blank
        fw = (self.eng.handle, self.table.handle, p(b.packets), self.n, p(b.inp), p(self.d_fw), p(self.d_status), s)
        nofw = fw[:5] + (None,) + fw[6:]
        rx = (self.eng.handle, self.index.handle, p(self.d_rx), None, self.n, p(self.d_rx_arena), p(self.d_route), p(self.d_via), s)
        for f, a in ((lib.neb_tx_resolve_batch, fw), (lib.neb_tx_resolve_batch, nofw), (lib.neb_rx_resolve_batch, rx)):
            L.check(f(*a), "bare call")
        return {"a_tx_resolve_fw": lambda: lib.neb_tx_resolve_batch(*fw), "a_tx_resolve": lambda: lib.neb_tx_resolve_batch(*nofw),
                "a_rx_resolve": lambda: lib.neb_rx_resolve_batch(*rx)}

    def bare_update(self):
        """neb_tx_table_update_hosts putting four hosts' own tunnels again, four others every call."""
        groups = [tx_hosts([(str(ipaddress.ip_address(0x0A010000 + h)), h) for h in range(k, k + 4)])
                  for k in range(0, self.nhosts - 3, 4)]
        s = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        args = [(self.table.handle, None, 0, g.ctypes.data_as(C.c_void_p), 4, s) for g in groups]
        turn = iter(range(1 << 62))
        return lambda: L.lib().neb_tx_table_update_hosts(*args[next(turn) % len(args)])

    def check(self):
        """The device resolve equals the caller-filled tunnels and the host form; both seals agree."""
        t = self.torch
        self.filled.seal()
        self.resolve_seal()
        t.cuda.synchronize()
        got = self.blank.packets.cpu().numpy().view(TX_PACKET_DTYPE)
        assert (got["tunnel"] == self.pk_filled["tunnel"]).all(), "the resolve's tunnels differ from the host form's"
        assert self.d_fw.cpu().numpy().tobytes() == self.h_fw.tobytes() and (self.d_status.cpu().numpy() == 0).all()
        assert bool(t.equal(self.filled.out, self.blank.out)) and int(self.blank.nwires.cpu()[0]) == self.nw
        assert bool((self.blank.pk_status == 0).all()) and bool((self.blank.wire_status == 0).all())
        self.index.resolve_device(self.d_rx, self.d_rx_arena, None, self.d_route, self.d_via)
        t.cuda.synchronize()
        assert (self.d_rx.cpu().numpy().view(L.RX_PACKET_DTYPE)["key_id"] == self.rx_want).all()

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
        self.table.close()
        self.index.close()
        for c in self.ciphers:
            L.lib().neb_cipher_destroy(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plain", type=int, default=65536)
    ap.add_argument("--tso", type=int, default=1456)
    ap.add_argument("--shapes", default="1:0,4096:64", help="hosts:routes, comma separated")
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed work per window, at least")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--measures", default="a,b,c")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("tx_resolve_bench: no GPU (this tool measures on the device only)")
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    measures = a.measures.split(",")
    lines = []

    def emit(case, measure, windows_us, **more):
        lines.append({"tool": "tx_resolve_bench", "measure": measure, "reads": case.kind, "mix": case.mix, "packets": case.n,
                      "wires": case.nw, "hosts": case.nhosts, "routes": case.nroutes,
                      "median_us": round(statistics.median(windows_us), 2), "windows_us": [round(x, 2) for x in windows_us],
                      "window_s": a.window, "device": torch.cuda.get_device_name(0),
                      "build": L.lib().neb_build_id().decode(), **more})
        print(json.dumps(lines[-1]), flush=True)

    with Engine(0, max(h for h, _ in shapes) + 64) as eng:
        for kind, n in (("plain", a.plain), ("tso", a.tso)):
            for nhosts, nroutes in shapes:
                for mix in ("in_network", "routed"):
                    if mix == "routed" and not nroutes:
                        continue
                    case = Case(eng, kind, n, nhosts, nroutes, mix)
                    try:
                        case.check()
                        if "a" in measures:  # the three calls alternate, window by window
                            calls = case.bare_calls()
                            res = {k: [] for k in calls}
                            for _ in range(a.windows):
                                for k, fn in calls.items():
                                    res[k].append(case.timed_launches(fn, a.window))
                            for k, v in res.items():
                                emit(case, k, [u for u, _ in v], launches_per_window=v[-1][1])
                        if "u" in measures and kind == "plain" and mix == "in_network" and nhosts >= 4:
                            live, cap = nhosts + nroutes, nhosts + max(nroutes, 1)
                            small, rebuilt = timed_updates(case.bare_update(), 4, live, max(16, 1 << (4 * cap - 1).bit_length()),
                                                           a.window, a.windows)
                            torch.cuda.synchronize()
                            emit(case, "u_update", small, clock="wall time of the calling thread")
                            emit(case, "u_rebuild", rebuilt, clock="wall time of the calling thread")
                            case.check()  # the table still resolves as before
                        if "b" in measures:  # alternating, step by step, until each form has its windows
                            forms = {"b_seal": case.filled.seal, "b_resolve_seal": case.resolve_seal}
                            done, acc, warm = {f: [] for f in forms}, {f: [0.0, 0] for f in forms}, 3
                            while any(len(v) < a.windows for v in done.values()):
                                for f, fn in forms.items():
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
                                emit(case, f, v[:a.windows])
                        if "c" in measures:
                            # the C entry point on arrays allocated and touched once, as a caller keeps them
                            host, ws = case.pk_blank.copy(), []
                            fw, st = np.zeros(case.n, L.FW_PACKET_DTYPE), np.zeros(case.n, np.int32)
                            vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
                            args = (case.table.handle, vp(host), case.n, vp(case.h_arena), case.h_arena.nbytes, vp(fw), vp(st))
                            L.check(L.lib().neb_tx_resolve_batch_host(*args), "neb_tx_resolve_batch_host")
                            assert fw.tobytes() == case.h_fw.tobytes() and (st == 0).all()
                            for _ in range(a.windows):
                                t0, calls_made = time.perf_counter(), 0
                                while time.perf_counter() - t0 < a.window:
                                    L.lib().neb_tx_resolve_batch_host(*args)
                                    calls_made += 1
                                ws.append((time.perf_counter() - t0) * 1e6 / calls_made)
                            emit(case, "c_host_form", ws, clock="wall time of one thread of the GPU box's host")
                    finally:
                        case.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
