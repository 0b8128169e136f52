"""GPU: the directed replay-window cases (tests/rxwin_cases.py; what they reach is pinned on the
CPU by tests/test_rxwin_cases.py) through every form of the batched receive, against
replay_oracle.rx_sequential and the AEAD oracle: statuses, every arena byte, and each window's
current, lost, dupe, out_of_window and whole bitmap, all exact.

Forms: the device receive held to its parallel form (NEB_KNOB_RX_STRICT) with mixed keys, the same
told its one key (key_hint), ChaCha20-Poly1305, the host receive rx_open_batch, and the device
receive free to finish on the host for the cases with forgeries or a tunnel without a window. The
sort's digits run on window slots that differ only in the low and only in the high digit, over
window sets of one to four passes."""
import random

import numpy as np
import pytest

import rxwin_cases as C
from nebula_amd import _lib as L

pytestmark = pytest.mark.gpu

from test_gpu_rx import SLOT, _build  # noqa: E402

CASES = C.cases()
STRICT = [n for n, c in CASES.items() if c.strict]
ONE_WINDOW = [n for n, c in CASES.items() if c.ntun == 1]
LOOSE = [n for n, c in CASES.items() if not c.strict]

_sealed = {}


def _material(oracle_mod, case, alg, keys):
    """(arena, descriptors with the tunnel in key_id, expected statuses, expected arena, the oracle's
    final windows), built once per case, algorithm and keys, and never changed."""
    key = (case.name, alg, tuple(keys))
    if key not in _sealed:
        arr = case.arrivals
        arena, desc, pts = _build(oracle_mod, alg, keys, arr, 5, lens=[0, 16])
        st, dec, wins, _ = case.replayed()
        exp = arena.copy()
        for i, ((t, _, forged), d) in enumerate(zip(arr, dec)):
            if d:  # it passed Check: decrypted in place, or wiped when its tag fails
                base = i * SLOT + 16
                exp[base:base + len(pts[i])] = 0 if forged else np.frombuffer(pts[i], np.uint8)
        arena.setflags(write=False)
        exp.setflags(write=False)
        _sealed[key] = (arena, desc, st, exp, wins)
    return _sealed[key]


def _install(engine, alg, case, want_slots=None):
    """One installed key per tunnel that has a window, the tunnels numbered in the order of the
    slots the allocator returned. want_slots: install keys until those slots are owned and use
    them. Returns (all ciphers, tunnel -> slot, the tunnels' keys)."""
    from nebula_amd.noiseutil import CipherAESGCM, CipherChaChaPoly

    cf = CipherAESGCM if alg == L.ALG_AESGCM else CipherChaChaPoly
    rng = random.Random(f"{case.name}/{alg}")
    present = [t for t in range(case.ntun) if t not in case.absent]
    held = []
    try:
        def more():
            k = rng.randbytes(32)
            held.append((cf.Cipher(engine, k), k))

        if want_slots is None:
            for _ in present:
                more()
            chosen = held
        else:
            while not set(want_slots) <= {c.key_id for c, _ in held}:
                assert len(held) < 2 * max(want_slots) + 8, "the allocator never returned the wanted slots"
                more()
            chosen = [ck for ck in held if ck[0].key_id in want_slots]
        chosen = sorted(chosen, key=lambda ck: ck[0].key_id)
        assert len(chosen) == len(present)
        slot_of = {t: c.key_id for t, (c, _) in zip(present, chosen)}
        keys = {t: k for t, (_, k) in zip(present, chosen)}
        for j, t in enumerate(sorted(case.absent)):
            slot_of[t] = engine.max_keys - 1 - j  # no window there
            keys[t] = rng.randbytes(32)
        return [c for c, _ in held], slot_of, [keys[t] for t in range(case.ntun)]
    except BaseException:
        for c, _ in held:
            c.destroy()
        raise


def _run(engine, oracle_mod, case, alg=L.ALG_AESGCM, form="device", count=None, hint=False, want_slots=None,
         measure=None):
    """form "device": neb_rx_open_batch on a DeviceWindows set of `count` slots ("fit": just the slots
    in use; None: engine.max_keys), every batch under its own strict flag; "host": rx_open_batch."""
    from nebula_amd.connection_state import Bits, DeviceWindows, rx_open_batch, rx_open_batch_device

    ciphers, slot_of, keys = _install(engine, alg, case, want_slots)
    dw = None
    try:
        arena0, desc, exp_status, exp_arena, owins = _material(oracle_mod, case, alg, keys)
        ewins = {}
        for t in owins:
            w = Bits(case.length)
            for c in case.history.get(t, []):
                w.Update(c)
            ewins[t] = w
        d = desc.copy()
        d["key_id"] = [slot_of[int(t)] for t in desc["key_id"]]
        arena = arena0.copy()
        got, a = [], 0
        if form == "device":
            import torch

            dev = torch.device("cuda", engine.device)
            if count == "fit":
                count = max(slot_of[t] for t in owins) + 1
            if measure is not None:
                torch.cuda.synchronize()
                measure.append(torch.cuda.mem_get_info(dev)[0])
            dw = DeviceWindows(engine, count or engine.max_keys, case.length)
            for t, w in ewins.items():
                dw.load(slot_of[t], w)
            d_arena = torch.from_numpy(arena).to(dev)
            key_hint = slot_of[case.arrivals[0][0]] if hint else L.KEYS_MIXED
            for arr, strict in case.batches:
                dd = torch.from_numpy(d[a:a + len(arr)].view(np.uint8).copy()).to(dev)
                st = torch.full((len(arr),), -1, dtype=torch.int32, device=dev)
                with L.knob(L.KNOB_RX_STRICT, 1 if strict else 0):
                    rx_open_batch_device(engine, alg, dw, dd, d_arena, st, key_hint=key_hint)
                torch.cuda.synchronize()
                got += st.cpu().tolist()
                a += len(arr)
            if measure is not None:
                measure.append(torch.cuda.mem_get_info(dev)[0])
            arena = d_arena.cpu().numpy()
            for t, w in ewins.items():
                dw.store(slot_of[t], w)
        else:
            windows = [None] * engine.max_keys
            for t, w in ewins.items():
                windows[slot_of[t]] = w
            for arr, _ in case.batches:
                got += rx_open_batch(engine, alg, windows, d[a:a + len(arr)], arena).tolist()
                a += len(arr)
        assert got == exp_status
        assert np.array_equal(arena, exp_arena)
        for t, w in ewins.items():
            o = owins[t]
            assert (w.current, w.lost, w.dupe, w.out_of_window) == (o.current, o.lost, o.dupe, o.out_of_window), t
            assert [bool(x) for x in w.snapshot()] == o.snapshot(), t
        return slot_of
    finally:
        if dw is not None:
            dw.destroy()
        for c in ciphers:
            c.destroy()


def _count_for(case):
    # arithmetic cases on a set of just their slots (at length 65536 a slot costs 16 KiB twice over)
    return "fit" if case.family == "arith" else None


@pytest.mark.parametrize("name", STRICT)
def test_parallel_form_mixed_keys(engine, oracle_mod, name):
    """Every strict case on the device, the host finish refused: the kernels alone."""
    _run(engine, oracle_mod, CASES[name], count=_count_for(CASES[name]))


@pytest.mark.parametrize("name", ONE_WINDOW)
def test_parallel_form_key_hint(engine, oracle_mod, name):
    """One window, the receive told its key: the sort's identity path and the single-key open."""
    _run(engine, oracle_mod, CASES[name], count="fit", hint=True)


@pytest.mark.parametrize("name", STRICT)
def test_parallel_form_chacha(engine, oracle_mod, name):
    _run(engine, oracle_mod, CASES[name], alg=L.ALG_CHACHAPOLY, count=_count_for(CASES[name]))


@pytest.mark.parametrize("name", list(CASES))
def test_host_form(engine, oracle_mod, name):
    _run(engine, oracle_mod, CASES[name], form="host")


@pytest.mark.parametrize("name", LOOSE)
def test_device_form_with_forgeries(engine, oracle_mod, name):
    """Forgeries in a role at an edge, and a tunnel without a window (BAD_KEY, bytes untouched, sorted
    last): the windows with a forgery finish on the host, the others on the device; a strict batch
    of the case stays strict."""
    _run(engine, oracle_mod, CASES[name])


# slots that differ only in the low digit (1, 2; 128, 129; 256, 257) and only in the high one
# (1, 129, 257; 128, 256), around the digit's edge (127, 128)
DIGIT_SLOTS = (1, 2, 127, 128, 129, 256, 257)


@pytest.mark.parametrize("count,length", [("fit", 1024), (None, 1024), (40000, 1024), ((1 << 21) + 1, 64)])
def test_sort_digits_and_passes(engine, oracle_mod, count, length):
    """pos_heads (seven windows) on the slots DIGIT_SLOTS, over window sets whose sort takes 2
    (engine.max_keys), 3 (40 000) and 4 passes (2^21 + 1 windows of length 64). The one-pass set has
    at most 255 slots and one digit, the whole key, so it runs on 1, 2, 3, 126, 127, 128 and 129.

    The 4-pass set took 202 MiB of device memory (torch.cuda.mem_get_info before the window set is
    created and after its batch: the set, the batch's workspace and its 3 MiB arena), against the
    0.2 GB estimated from rx_ws_layout and neb_dwindows_create; the 1-, 2- and 3-pass sets 14, 20
    and 30 MiB. Five passes would need 2^28 windows, tens of GB of window state, and are left out."""
    case = CASES[f"pos_heads_{length}"]
    digit = C.constants()["sort_digit"]
    want = DIGIT_SLOTS if count != "fit" else (1, 2, 3, 126, 127, 128, 129)
    assert len(want) == case.ntun
    measure = []
    slot_of = _run(engine, oracle_mod, case, count=count, want_slots=want, measure=measure)
    got = sorted(slot_of.values())
    pairs = [(a, b) for a in got for b in got if a < b]
    assert any(a >> digit == b >> digit for a, b in pairs), got  # only the low digit differs
    if count != "fit":  # only the high digit differs
        assert any(a >> digit != b >> digit and (a ^ b) & ((1 << digit) - 1) == 0 for a, b in pairs), got
    nwin = {"fit": max(got) + 1, None: engine.max_keys}.get(count, count)
    passes = 1 if nwin.bit_length() <= 8 else -(-nwin.bit_length() // digit)
    assert passes == {"fit": 1, None: 2, 40000: 3, (1 << 21) + 1: 4}[count]
    print(f"window set of {nwin} x {length}: {passes} passes, {(measure[0] - measure[1]) / 2**20:.1f} MiB")
