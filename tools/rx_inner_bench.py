"""What the RX inner resolve (neb_rx_inner_batch) costs on a device-resident batch, beside the call
whose place it takes and the pipeline it sits in.

Workload: --n wire packets (default 64 Ki) of 1364 bytes in slots of 1408, each a 1332-byte TCP/IPv4
segment from its tunnel's VPN address (10.1.x.y) to an address of its own (10.3.x.y) inside a routable
network of the node, the tunnels' segments in flow order so the coalescer has its usual work. Table
states: 1 tunnel with its one entry, and 4096 tunnels with their VPN entry plus ten unsafe prefixes
each (/0 /1 /8 /24 /31 /32, /48 /64 /127 /128). Measures, per state:

  a_inner            neb_rx_inner_batch alone on an opened batch (device events around a run of launches),
  a_plain_from_wire  neb_rx_plain_from_wire alone on the same batch, and
  a_tx_resolve       neb_tx_resolve_batch alone on the same plaintexts read as TUN reads: the own network
                     is around the destinations, every destination has a host entry, and the TX table
                     has the peer table's capacity and as many live entries, so both calls walk one
                     chain per packet, the tunnels' packets at different slots of a table of the same
                     footprint; window by window in turn
  b_pipeline_plain   neb_rx_open_wire_batch -> neb_rx_plain_from_wire -> neb_rx_coalesce_batch, against
  b_pipeline_inner   the same with neb_rx_inner_batch in the middle, alternating step by step; the
                     packets are re-sealed on the device outside the timed window
  c_host_form        neb_rx_inner_batch_host's C entry point on one thread over the opened arena, into
                     output arrays allocated once (wall time of the calling thread)
  d_through_host     the same checks composed by the caller: the first 96 bytes of every packet copied
                     to the host, the same C entry point over them, one flag per packet uploaded (wall
                     time)

Every figure is the median over windows of at least --window seconds of timed work. Before timing the
device form must equal the host form, and every packet must pass.

  python tools/rx_inner_bench.py --out profiles/rx_inner/bench.jsonl
"""
import argparse
import ctypes as C
import json
import os
import statistics
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from nebula_amd import _lib as L  # noqa: E402
from nebula_amd import outside as O  # noqa: E402
from nebula_amd.connection_state import Bits, DeviceWindows, rx_open_wire_batch_device  # noqa: E402
from nebula_amd.hostmap import PeerTable, TxTable, peer_nets  # noqa: E402
from nebula_amd.inside import TX_PACKET_DTYPE  # noqa: E402
from nebula_amd.noiseutil import Engine  # noqa: E402

WIRE, STRIDE, PAYLOAD, HEAD = 1364, 1408, 1364 - 32, 96
NEST = [("0.0.0.0/0", L.NET_UNSAFE), ("128.0.0.0/1", L.NET_UNSAFE), ("200.0.0.0/8", L.NET_UNSAFE), ("200.1.2.0/24", L.NET_UNSAFE),
        ("200.1.2.4/31", L.NET_UNSAFE), ("200.1.2.5/32", L.NET_UNSAFE), ("2001:db8:1::/48", L.NET_UNSAFE),
        ("2001:db8:1:2::/64", L.NET_UNSAFE), ("2001:db8:1:2::4/127", L.NET_UNSAFE), ("2001:db8:1:2::5/128", L.NET_UNSAFE)]


class Case:
    def __init__(self, eng, alg, n, ntun, nest):
        import torch

        self.torch, self.eng, self.alg, self.n, self.ntun = torch, eng, alg, n, ntun
        self.dev = torch.device("cuda", eng.device)
        rng = np.random.default_rng(1)
        keys = rng.integers(0, 256, (ntun, 32), dtype=np.uint8)
        out = (C.c_void_p * ntun)()
        L.check(L.lib().neb_cipher_create_batch(eng.handle, alg, keys.ctypes.data_as(C.c_void_p), ntun, out), "neb_cipher_create_batch")
        self.ciphers = [C.c_void_p(h) for h in out]
        self.kid = np.array([L.lib().neb_cipher_key_id(c) for c in self.ciphers], np.uint32)
        i = np.arange(n)
        self.tt = (i % ntun).astype(np.uint32)  # interleaved tunnels
        self.place, self.per = (i // ntun).astype(np.uint64), -(-n // ntun)
        self.off = (i * STRIDE).astype(np.uint64)
        self.hint = int(self.kid[0]) if ntun == 1 else L.KEYS_MIXED
        # plaintext: IPv4 (DF) + TCP (ACK), 1292 payload bytes, the tunnel's segments in sequence
        pay = PAYLOAD - 40
        rows = rng.integers(0, 256, (n, STRIDE), dtype=np.uint8)
        ip = np.zeros((n, 40), np.uint8)
        ip[:, 0], ip[:, 6], ip[:, 8], ip[:, 9] = 0x45, 0x40, 64, 6
        ip[:, 2:4] = np.frombuffer(struct.pack(">H", PAYLOAD), np.uint8)
        ip[:, 12], ip[:, 13] = 10, 1
        ip[:, 14], ip[:, 15] = 16 + self.tt // 256, self.tt % 256
        ip[:, 16], ip[:, 17] = 10, 3
        ip[:, 18], ip[:, 19] = 16 + self.tt // 256, self.tt % 256
        ip[:, 20:22], ip[:, 22:24] = np.frombuffer(struct.pack(">H", 40000), np.uint8), np.frombuffer(struct.pack(">H", 443), np.uint8)
        ip[:, 24:28] = (1000 + self.place * pay).astype(">u4").reshape(-1, 1).view(np.uint8)
        ip[:, 32], ip[:, 33] = 5 << 4, 0x10
        rows[:, 16:56] = ip
        self.arena = torch.from_numpy(rows.reshape(-1)).to(self.dev)
        self.rows = self.arena.view(n, STRIDE)
        pk = np.zeros(n, L.RX_PACKET_DTYPE)
        pk["off"], pk["len"], pk["key_id"] = self.off, WIRE, self.kid[self.tt]
        self.pk = pk
        nslots = int(self.kid.max()) + 1
        self.epoch = np.ones(nslots, np.uint64)
        self.peers = PeerTable(eng, ntun * (1 + len(NEST)) if nest else ntun)
        self.peers.set_routable(["10.1.0.7/32", "10.3.0.0/16"])
        one = peer_nets([(0, "10.1.16.0/32", L.NET_VPN)] + ([(0, p, ty) for p, ty in NEST] if nest else []))
        nets = np.tile(one, ntun)
        nets["tunnel"] = np.repeat(self.kid, len(one))
        own = np.arange(ntun) * len(one)
        nets["addr"][own, 2], nets["addr"][own, 3] = 16 + np.arange(ntun) // 256, np.arange(ntun) % 256
        self.peers.update(put=nets)
        self.entries = len(nets)
        # the comparator's table: the peer table's capacity, as many live host entries, the
        # destinations among them
        hosts = np.zeros(len(nets), L.TX_HOST_DTYPE)
        j = np.arange(len(nets))
        hosts["family"], hosts["tunnel"] = 4, j % 16
        hosts["addr"][:, 0], hosts["addr"][:, 1] = 10, 4 + j // 65536
        hosts["addr"][:, 2], hosts["addr"][:, 3] = (j // 256) % 256, j % 256
        hosts["addr"][own, 1], hosts["addr"][own, 2], hosts["addr"][own, 3] = 3, 16 + np.arange(ntun) // 256, np.arange(ntun) % 256
        self.tx = TxTable(eng, len(nets))
        self.tx.set_own(["10.3.255.254/16"], True, True)
        self.tx.update_hosts([], hosts)
        txp = np.zeros(n, TX_PACKET_DTYPE)
        txp["in_off"], txp["len"] = self.off + np.uint64(16), PAYLOAD
        z = lambda k, dt=torch.uint8: torch.zeros(k, dtype=dt, device=self.dev)  # noqa: E731
        self.d_pk, self.d_tx, self.d_epoch = self.up(pk), self.up(txp), self.up(self.epoch).view(torch.int64)
        self.d_status, self.d_sub, self.d_inner, self.d_txst = (z(n, torch.int32) for _ in range(4))
        self.d_plain, self.d_fw = z(n * 32), z(n * 48)
        self.cap = n * ((PAYLOAD + 15) & ~15)
        self.d_out, self.d_writes = z(self.cap), z(n * 32)
        self.d_nw, self.d_pw, self.d_ps = z(1, torch.int32), z(n, torch.int32), z(n, torch.int32)
        self.dw = DeviceWindows(eng, eng.max_keys, 8192)
        w = Bits(8192)
        for k in self.kid:
            self.dw.load(int(k), w)
        self.step = 0

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev)

    def prepare(self):
        """Untimed: the plaintexts sealed in place with fresh counters."""
        self.step += 1
        c = np.uint64(self.step * self.per) + self.place + np.uint64(1)
        h = np.zeros((self.n, 16), np.uint8)
        h[:, 0] = 0x11
        h[:, 8:16] = c.astype(">u8").reshape(-1, 1).view(np.uint8)
        self.rows[:, :16] = self.up(h).view(self.n, 16)
        d = np.zeros(self.n, L.DESC_DTYPE)
        d["aad_off"], d["aad_len"] = self.off, 16
        d["src_off"] = d["dst_off"] = self.off + np.uint64(16)
        d["len"], d["counter"], d["key_id"] = PAYLOAD, c, self.kid[self.tt]
        dd = self.up(d)
        s = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        L.check(L.lib().neb_seal_batch(self.eng.handle, self.alg, C.c_void_p(dd.data_ptr()), self.n, C.c_void_p(self.arena.data_ptr()),
                                       C.c_void_p(self.d_sub.data_ptr()), self.hint, s), "neb_seal_batch")
        self.torch.cuda.synchronize()

    def pipeline(self, inner):
        rx_open_wire_batch_device(self.eng, self.alg, self.dw, self.d_pk, self.arena, self.d_status, self.hint)
        if inner:
            O.inner_device(self.eng, self.peers, self.d_pk, self.d_status, self.d_epoch, self.arena, self.d_plain, self.d_fw, self.d_inner)
        else:
            O.plain_from_wire_device(self.eng, self.d_pk, self.d_status, self.d_epoch, self.arena, self.d_plain)
        O.coalesce_batch_device(self.eng, self.d_plain, self.arena, self.d_out, self.d_writes, self.d_nw, self.d_pw, self.d_ps)

    def bare_calls(self):
        """The three enqueue-only calls with their arguments built once."""
        lib, p = L.lib(), lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        s = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        ia = (self.eng.handle, self.peers.handle, p(self.d_pk), p(self.d_status), p(self.d_epoch), self.d_epoch.numel(), self.n,
              p(self.arena), p(self.d_plain), p(self.d_fw), p(self.d_inner), s)
        pa = (self.eng.handle, p(self.d_pk), p(self.d_status), p(self.d_epoch), self.d_epoch.numel(), self.n, p(self.arena),
              p(self.d_plain), s)
        ta = (self.eng.handle, self.tx.handle, p(self.d_tx), self.n, p(self.arena), p(self.d_fw), p(self.d_txst), s)
        calls = {"a_inner": lambda: lib.neb_rx_inner_batch(*ia), "a_plain_from_wire": lambda: lib.neb_rx_plain_from_wire(*pa),
                 "a_tx_resolve": lambda: lib.neb_tx_resolve_batch(*ta)}
        for name, fn in calls.items():
            L.check(fn(), name)
        self.torch.cuda.synchronize()
        assert bool((self.d_txst == 0).all()), "the TX resolve comparator does not resolve every read"
        return calls

    def check(self):
        """The batch opens, every packet passes, the device form equals the host form, the coalescer
        writes the same bytes behind either middle step."""
        t = self.torch
        self.prepare()
        self.pipeline(False)
        t.cuda.synchronize()
        assert bool((self.d_status == 0).all()), "a packet did not open"
        ref = (int(self.d_nw.item()), self.d_writes.cpu().numpy().tobytes(), self.d_pw.cpu().numpy().tobytes())
        self.prepare()
        self.pipeline(True)
        t.cuda.synchronize()
        assert bool((self.d_inner == 0).all()), "a packet was refused"
        got = (int(self.d_nw.item()), self.d_writes.cpu().numpy().tobytes(), self.d_pw.cpu().numpy().tobytes())
        assert got == ref, "the pipeline's writes differ between the two middle steps"
        self.h_arena = self.arena.cpu().numpy()
        plain, fw, st = O.inner_host(self.peers, self.pk, np.zeros(self.n, np.int32), self.epoch, self.h_arena)
        assert not st.any()
        assert plain.tobytes() == self.d_plain.cpu().numpy().tobytes() and fw.tobytes() == self.d_fw.cpu().numpy().tobytes()
        return ref[0]

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
        self.peers.close()
        self.tx.close()
        self.dw.destroy()
        for c in self.ciphers:
            L.lib().neb_cipher_destroy(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--shapes", default="1:0,4096:1", help="tunnels:unsafe prefixes (0 | 1), comma separated")
    ap.add_argument("--alg", default="aesgcm")
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed work per window, at least")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--measures", default="a,b,c,d")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("rx_inner_bench: no GPU (this tool measures on the device only)")
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]
    measures = a.measures.split(",")
    alg = L.ALG_AESGCM if a.alg == "aesgcm" else L.ALG_CHACHAPOLY
    lines = []

    def emit(case, measure, windows_us, **more):
        lines.append({"tool": "rx_inner_bench", "measure": measure, "alg": a.alg, "packets": case.n, "tunnels": case.ntun,
                      "table_entries": case.entries, "wire_bytes": WIRE, "median_us": round(statistics.median(windows_us), 2),
                      "windows_us": [round(x, 2) for x in windows_us], "window_s": a.window, "device": torch.cuda.get_device_name(0),
                      "build": L.lib().neb_build_id().decode(), **more})
        print(json.dumps(lines[-1]), flush=True)

    with Engine(0, max(t for t, _ in shapes) + 64) as eng:
        for ntun, nest in shapes:
            case = Case(eng, alg, a.n, ntun, bool(nest))
            try:
                nwrites = case.check()
                if "b" in measures:  # alternating, step by step, until each form has its windows
                    forms = {"b_pipeline_plain": False, "b_pipeline_inner": True}
                    done, acc, warm = {f: [] for f in forms}, {f: [0.0, 0] for f in forms}, 3
                    while any(len(v) < a.windows for v in done.values()):
                        for f, inner in forms.items():
                            case.prepare()
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            case.pipeline(inner)
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
                        emit(case, f, v[:a.windows], tun_writes=nwrites)
                case.prepare()
                case.pipeline(True)  # an opened batch with its statuses, for a, c and d
                torch.cuda.synchronize()
                if "a" in measures:
                    calls = case.bare_calls()
                    res = {k: [] for k in calls}
                    for _ in range(a.windows):  # the three alternate, window by window
                        for k, fn in calls.items():
                            res[k].append(case.timed_launches(fn, a.window))
                    for k, v in res.items():
                        emit(case, k, [u for u, _ in v], launches_per_window=v[-1][1])
                h_arena = case.arena.cpu().numpy()
                zeros = np.zeros(case.n, np.int32)
                vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
                o_plain, o_st = np.zeros(case.n, L.PLAIN_PACKET_DTYPE), np.zeros(case.n, np.int32)
                o_fw = np.zeros(case.n, L.FW_PACKET_DTYPE)

                def host_form(pk, arena, fw):
                    L.check(L.lib().neb_rx_inner_batch_host(case.peers.handle, vp(pk), vp(zeros), vp(case.epoch), len(case.epoch),
                                                            case.n, vp(arena), arena.nbytes, vp(o_plain), fw, vp(o_st)),
                            "neb_rx_inner_batch_host")
                if "c" in measures:
                    ws = []
                    for _ in range(a.windows):
                        t0, calls_ = time.perf_counter(), 0
                        while time.perf_counter() - t0 < a.window:
                            host_form(case.pk, h_arena, vp(o_fw))
                            calls_ += 1
                        ws.append((time.perf_counter() - t0) * 1e6 / calls_)
                    assert not o_st.any()
                    emit(case, "c_host_form", ws, clock="wall time of the calling thread on the GPU box's host, outputs allocated once")
                if "d" in measures:
                    heads = torch.empty((case.n, HEAD), dtype=torch.uint8).pin_memory()
                    flags = torch.empty(case.n, dtype=torch.int32).pin_memory()
                    d_flags = torch.zeros(case.n, dtype=torch.int32, device=case.dev)
                    hp = np.zeros(case.n, L.RX_PACKET_DTYPE)
                    hp["off"], hp["len"], hp["key_id"] = np.arange(case.n, dtype=np.uint64) * HEAD, HEAD, case.pk["key_id"]
                    h_heads = heads.numpy().reshape(-1)
                    ws = []
                    for _ in range(a.windows):
                        t0, calls_ = time.perf_counter(), 0
                        while time.perf_counter() - t0 < a.window:
                            heads.copy_(case.rows[:, :HEAD], non_blocking=True)
                            torch.cuda.synchronize()
                            host_form(hp, h_heads, None)
                            flags.numpy()[:] = o_st
                            d_flags.copy_(flags, non_blocking=True)
                            torch.cuda.synchronize()
                            calls_ += 1
                        ws.append((time.perf_counter() - t0) * 1e6 / calls_)
                    assert bool((d_flags == 0).all())
                    emit(case, "d_through_host", ws, clock="wall time: D2H of 96-byte heads, host form's C entry point, H2D of flags", head_bytes=HEAD)
            finally:
                case.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
