"""What the RX receive plan (neb_rx_recv_plan) costs on a device-resident receive batch, beside the
resolve and the open it feeds, the host loop it replaces and the descriptor upload it saves.

Workload: wire packets of 1364 bytes (AES-256-GCM, 64 tunnels, one source address each) lying back to
back in the arena as UDP_GRO leaves them, described by receive entries in three shapes:

  1024x64   1024 entries of 64 segments (65 536 packets)
  65536x1   65 536 entries of one packet (65 536 packets)
  skew      one entry of 65 535 packets in the middle of 1024 one-packet entries (66 559 packets)

Measures, per shape:

  a_plan        neb_rx_recv_plan alone over max_packets = the packets, with control buffers (stride 24,
                one UDP_GRO cmsg) and with seg_size (device events around a run of calls)
  b_prebuilt    neb_rx_resolve_batch + neb_rx_open_wire_batch over descriptors built beforehand, against
  b_planned     the plan in front of the same two calls on the same stream, alternating step by step on
                freshly sealed packets; delta_us is the difference of the medians
  c_host_form   neb_rx_recv_plan_host's C entry point on one thread, outputs allocated once (wall time)
  d_upload      the per-packet descriptors the plan replaces (36 B x packets) copied from pinned host
                memory to the device, against the entries (48 B x entries) and the entries with their
                control slots (wall time, each copy ended by a synchronise)

a, c and d: the median over windows of at least --window seconds of timed work; b: the median, the
least and the most over --steps steps per form. Before timing the device form must equal the host form
and the planned batch must open every packet.

  python tools/recv_plan_bench.py --out profiles/recv_plan/bench.jsonl
  rocprofv3 --kernel-trace --stats ... -- python tools/recv_plan_bench.py --measures a --window 0.02 --windows 1
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
from nebula_amd import _lib as L  # noqa: E402
from nebula_amd.connection_state import Bits, DeviceWindows  # noqa: E402
from nebula_amd.hostmap import IndexTable  # noqa: E402
from nebula_amd.noiseutil import Engine  # noqa: E402

WIRE, PAYLOAD, NTUN, STRIDE = 1364, 1364 - 32, 64, 24
SHAPES = {"1024x64": [64] * 1024, "65536x1": [1] * 65536, "skew": [1] * 512 + [65535] + [1] * 512}


def headers(remote_index, counters):
    """header.Encode(1, Message, 0, remote_index, counter) for arrays -> (n, 16) uint8"""
    h = np.zeros((len(counters), 16), np.uint8)
    h[:, 0] = 0x11
    h[:, 4:8] = np.asarray(remote_index, ">u4").reshape(-1, 1).view(np.uint8)
    h[:, 8:16] = np.asarray(counters, ">u8").reshape(-1, 1).view(np.uint8)
    return h


class Keys:
    def __init__(self, eng, alg, seed=1):
        rng = np.random.default_rng(seed)
        keys = rng.integers(0, 256, (NTUN, 32), dtype=np.uint8)
        out = (C.c_void_p * NTUN)()
        L.check(L.lib().neb_cipher_create_batch(eng.handle, alg, keys.ctypes.data_as(C.c_void_p), NTUN, out),
                "neb_cipher_create_batch")
        self.ciphers = [C.c_void_p(h) for h in out]
        self.kid = np.array([L.lib().neb_cipher_key_id(c) for c in self.ciphers], np.uint32)
        self.index = rng.permutation(1 << 20)[:NTUN].astype(np.uint32) + np.uint32(0x20000000)
        self.table = IndexTable(eng, NTUN)
        rows = np.zeros(NTUN, L.INDEX_ENTRY_DTYPE)
        rows["index"], rows["space"], rows["key_id"], rows["tunnel"] = self.index, L.INDEX_TUNNEL, self.kid, L.RELAY_NONE
        self.table.update([], rows)

    def close(self):
        self.table.close()
        for c in self.ciphers:
            L.lib().neb_cipher_destroy(c)


class Case:
    def __init__(self, eng, alg, keys, name):
        import torch

        self.torch, self.eng, self.alg, self.keys, self.name = torch, eng, alg, keys, name
        self.dev = torch.device("cuda", eng.device)
        counts = np.array(SHAPES[name], np.int64)
        self.ne, self.n = len(counts), int(counts.sum())
        first = np.concatenate([[0], np.cumsum(counts)[:-1]])
        etun = (np.arange(self.ne) % NTUN).astype(np.uint32)
        # the entries: a v6 socket, tunnel t's packets come from 2001:db8::t, port 4242 + t
        en = np.zeros(self.ne, L.RECV_ENTRY_DTYPE)
        en["off"], en["len"] = first * WIRE, counts * WIRE
        en["seg_size"] = np.where(counts > 1, WIRE, 0)
        en["name"][:, 0] = 10
        en["name"][:, 2:4] = (4242 + etun).astype(">u2").reshape(-1, 1).view(np.uint8)
        en["name"][:, 8:12] = [0x20, 0x01, 0x0d, 0xb8]
        en["name"][:, 23] = etun
        en["ctrl_len"] = np.where(counts > 1, STRIDE, 0)
        ctrl = np.zeros((self.ne, STRIDE), np.uint8)
        ctrl[:, 0], ctrl[:, 8], ctrl[:, 12] = 20, 17, 104  # cmsghdr {20, SOL_UDP, UDP_GRO}
        ctrl[:, 16:20] = np.array([WIRE], "<i4").view(np.uint8)
        self.en, self.ctrl = en, ctrl.reshape(-1)
        # the packets
        self.tt = np.repeat(etun, counts)
        order = np.argsort(self.tt, kind="stable")
        place = np.empty(self.n, np.uint64)
        start = np.concatenate([[0], np.cumsum(np.bincount(self.tt, minlength=NTUN))[:-1]])
        place[order] = np.arange(self.n) - np.repeat(start, np.bincount(self.tt, minlength=NTUN))
        self.place, self.per = place, int(np.bincount(self.tt).max())
        self.off = (np.arange(self.n) * WIRE).astype(np.uint64)
        pk = np.zeros(self.n, L.RX_PACKET_DTYPE)
        pk["off"], pk["len"], pk["key_id"] = self.off, WIRE, L.KEYS_MIXED
        src = np.zeros(self.n, L.RX_SOURCE_DTYPE)
        src["addr"] = np.repeat(en["name"][:, 8:24], counts, axis=0)
        src["family"] = 6
        self.pk, self.src = pk, src
        self.arena = torch.zeros(self.n * WIRE + 64, dtype=torch.uint8, device=self.dev)
        self.d_en, self.d_ctrl = self.up(en), self.up(self.ctrl)
        self.d_pk, self.d_src = self.up(pk), self.up(src)
        z = lambda count, item=1, dt=torch.uint8: torch.zeros(max(count, 1) * item, dtype=dt, device=self.dev)  # noqa: E731
        self.o_pk, self.o_src, self.o_pe = z(self.n, 16), z(self.n, 20), z(self.n, 1, torch.int32)
        self.o_from, self.o_first, self.o_cnt = z(self.ne, 20), z(self.ne, 1, torch.int32), z(2, 1, torch.int32)
        self.d_status, self.d_sub = z(self.n, 1, torch.int32), z(self.n, 1, torch.int32)
        self.dw = DeviceWindows(eng, eng.max_keys, 8192)
        w = Bits(8192)
        for k in keys.kid:
            self.dw.load(int(k), w)
        self.step = 0

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev)

    def prepare(self):
        """Untimed: this step's datagrams, sealed in place with fresh counters."""
        self.step += 1
        c = np.uint64(self.step * self.per) + self.place + np.uint64(1)
        hdr = self.up(headers(self.keys.index[self.tt], c)).view(self.n, 16)
        rows = self.arena[:self.n * WIRE].view(self.n, WIRE)
        rows[:, :16] = hdr
        d = np.zeros(self.n, L.DESC_DTYPE)
        d["aad_off"], d["aad_len"] = self.off, 16
        d["src_off"] = d["dst_off"] = self.off + np.uint64(16)
        d["len"], d["counter"], d["key_id"] = PAYLOAD, c, self.keys.kid[self.tt]
        dd = self.up(d)
        s = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        L.check(L.lib().neb_seal_batch(self.eng.handle, self.alg, C.c_void_p(dd.data_ptr()), self.n,
                                       C.c_void_p(self.arena.data_ptr()), C.c_void_p(self.d_sub.data_ptr()), L.KEYS_MIXED, s),
                "neb_seal_batch")
        self.torch.cuda.synchronize()

    def bare(self):
        """The calls with their arguments built once: the timed runs pay the C call and the launches,
        not a Python wrapper. Returns (plan with ctrl, plan with seg_size, resolve + open over the
        plan's records, resolve + open over the descriptors built beforehand)."""
        lib, p = L.lib(), lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        s = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        h, e = self.eng.handle, self

        def plan_args(ctrl):
            return (h, p(e.d_en), e.ne, p(e.d_ctrl) if ctrl else None, STRIDE, 0, p(e.o_pk), p(e.o_src), p(e.o_pe), e.n,
                    p(e.o_from), p(e.o_first), p(e.o_cnt), s)

        def rest_args(d_pk, d_src):
            return ((h, e.keys.table.handle, p(d_pk), p(d_src), e.n, p(e.arena), None, None, s),
                    (h, e.alg, e.dw.handle, p(d_pk), e.n, p(e.arena), p(e.d_status), L.KEYS_MIXED, s))

        def rest(d_pk, d_src):
            ra, oa = rest_args(d_pk, d_src)

            def run():
                lib.neb_rx_resolve_batch(*ra)
                lib.neb_rx_open_wire_batch(*oa)
            return run

        pc, ps = plan_args(True), plan_args(False)
        return (lambda: lib.neb_rx_recv_plan(*pc)), (lambda: lib.neb_rx_recv_plan(*ps)), rest(self.o_pk, self.o_src), \
            rest(self.d_pk, self.d_src)

    def host_args(self, ctrl):
        vp = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
        o = {"pk": np.zeros(self.n, L.RX_PACKET_DTYPE), "src": np.zeros(self.n, L.RX_SOURCE_DTYPE),
             "pe": np.zeros(self.n, np.uint32), "from": np.zeros(self.ne, L.UDP_ADDR_DTYPE),
             "first": np.zeros(self.ne, np.uint32), "cnt": np.zeros(2, np.uint32)}
        args = (vp(self.en), self.ne, vp(self.ctrl) if ctrl else None, STRIDE, 0, vp(o["pk"]), vp(o["src"]), vp(o["pe"]), self.n,
                vp(o["from"]), vp(o["first"]), vp(o["cnt"]))
        return o, args

    def check(self):
        """Both device modes equal the host form, which names the packets as laid out; the planned
        batch opens every packet, and so does the prebuilt one."""
        t = self.torch
        plan_c, plan_s, rest_planned, rest_prebuilt = self.bare()
        for ctrl, call in ((True, plan_c), (False, plan_s)):
            o, args = self.host_args(ctrl)
            L.check(L.lib().neb_rx_recv_plan_host(*args), "neb_rx_recv_plan_host")
            assert o["cnt"].tolist() == [self.n, self.ne]
            assert o["pk"].tobytes() == self.pk.tobytes() and o["src"].tobytes() == self.src.tobytes()
            for x in (self.o_pk, self.o_src, self.o_pe, self.o_from, self.o_first, self.o_cnt):
                x.fill_(0x5A)
            L.check(call(), "neb_rx_recv_plan")
            t.cuda.synchronize()
            for name, d in (("pk", self.o_pk), ("src", self.o_src), ("pe", self.o_pe), ("from", self.o_from),
                            ("first", self.o_first), ("cnt", self.o_cnt)):
                assert d.cpu().numpy().view(np.uint8).tobytes() == o[name].tobytes(), (self.name, ctrl, name)
        for planned in (True, False):
            self.prepare()
            if planned:
                plan_c()
                rest_planned()
            else:
                rest_prebuilt()
            t.cuda.synchronize()
            assert (self.d_status == 0).all().item(), (self.name, planned)

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
        self.dw.destroy()


def wall(fn, window, windows):
    out = []
    for _ in range(windows):
        t0, calls = time.perf_counter(), 0
        while time.perf_counter() - t0 < window:
            fn()
            calls += 1
        out.append((time.perf_counter() - t0) * 1e6 / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1024x64,65536x1,skew")
    ap.add_argument("--window", type=float, default=0.5, help="seconds of timed work per window, at least")
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30, help="b: timed steps per form")
    ap.add_argument("--measures", default="a,b,c,d")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("recv_plan_bench: no GPU (this tool measures on the device only)")
    measures = a.measures.split(",")
    lines = []

    def emit(case, measure, us, **more):
        lines.append({"tool": "recv_plan_bench", "measure": measure, "shape": case.name, "entries": case.ne, "packets": case.n,
                      "wire_bytes": WIRE, "median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2),
                      "max_us": round(max(us), 2), "samples": len(us), "device": torch.cuda.get_device_name(0),
                      "build": L.lib().neb_build_id().decode(), **more})
        print(json.dumps(lines[-1]), flush=True)

    alg = L.ALG_AESGCM
    with Engine(0, NTUN + 64) as eng:
        keys = Keys(eng, alg)
        try:
            for name in a.shapes.split(","):
                case = Case(eng, alg, keys, name)
                try:
                    case.check()
                    plan_c, plan_s, rest_planned, rest_prebuilt = case.bare()
                    if "a" in measures:
                        for mode, call in (("ctrl", plan_c), ("seg_size", plan_s)):
                            res = [case.timed_launches(call, a.window) for _ in range(a.windows)]
                            emit(case, "a_plan", [u for u, _ in res], size_from=mode, window_s=a.window,
                                 launches_per_window=res[-1][1])
                    if "b" in measures:  # alternating, step by step, on freshly sealed packets
                        got = {"b_prebuilt": [], "b_planned": []}
                        for step in range(a.steps + 3):
                            for form in got:
                                case.prepare()
                                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                                e0.record()
                                if form == "b_planned":
                                    plan_c()
                                    rest_planned()
                                else:
                                    rest_prebuilt()
                                e1.record()
                                e1.synchronize()
                                assert (case.d_status == 0).all().item()
                                if step >= 3:
                                    got[form].append(e0.elapsed_time(e1) * 1e3)
                        base = statistics.median(got["b_prebuilt"])
                        emit(case, "b_prebuilt", got["b_prebuilt"])
                        emit(case, "b_planned", got["b_planned"], size_from="ctrl",
                             delta_us=round(statistics.median(got["b_planned"]) - base, 2))
                    if "c" in measures:
                        for mode in (True, False):
                            _, args = case.host_args(mode)
                            emit(case, "c_host_form", wall(lambda: L.lib().neb_rx_recv_plan_host(*args), a.window, a.windows),
                                 size_from="ctrl" if mode else "seg_size", window_s=a.window,
                                 clock="wall time of the calling thread on the GPU machine's host, outputs allocated once")
                    if "d" in measures:
                        def upload(parts):
                            pinned = [torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).pin_memory()
                                      for x in parts]
                            dst = [torch.empty_like(x, device=case.dev) for x in pinned]

                            def run():
                                for d, s in zip(dst, pinned):
                                    d.copy_(s, non_blocking=True)
                                torch.cuda.synchronize()
                            return run, sum(x.numel() for x in pinned)
                        for what, parts in (("descriptors", (case.pk, case.src)), ("entries", (case.en,)),
                                            ("entries_and_ctrl", (case.en, case.ctrl))):
                            run, nbytes = upload(parts)
                            emit(case, "d_upload", wall(run, a.window, a.windows), what=what, bytes=nbytes, window_s=a.window,
                                 clock="wall time: H2D from pinned memory, each copy ended by a synchronise")
                finally:
                    case.close()
        finally:
            keys.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
