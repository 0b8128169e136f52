"""CPU: the connection table's host form (neb_conntrack_*_host on a host-only table, conntrack.cpp
over conntrack_core.hpp) against the model (tests/conntrack_ref.py) on random scripts of mixed
operations, with the image compared after every step; the new symbols are exported; argument checks."""
import ctypes as C

import numpy as np
import pytest

from nebula_amd import _lib as L
from nebula_amd import firewall as F

import conntrack_cases as K
import conntrack_ref as R

SIZES = [1, 63, 64, 65, 255, 256, 257]
SYMBOLS = ["neb_conntrack_create", "neb_conntrack_destroy", "neb_conntrack_set_rules_version", "neb_conntrack_lookup_batch",
           "neb_conntrack_lookup_batch_host", "neb_conntrack_add_batch", "neb_conntrack_add_batch_host",
           "neb_conntrack_evict_batch", "neb_conntrack_evict_batch_host", "neb_conntrack_compact", "neb_conntrack_count",
           "neb_conntrack_home", "neb_conntrack_dump"]


def test_every_new_symbol_is_exported():
    lib = L.lib()
    for s in SYMBOLS:
        assert hasattr(lib, s) and s in L.SIGNATURES, s
    assert L.STATUS_FW_HELD == 18 and L.CT_WORK_DTYPE.itemsize == 64 and L.CT_SLOT_DTYPE.itemsize == 64


@pytest.mark.parametrize("capacity", [1, 4, 1024])
def test_random_scripts_against_the_model(capacity):
    rng = np.random.default_rng(capacity)
    keys = K.universe(capacity + 3 if capacity < 1024 else 1400)  # more keys than places: FULL happens
    with F.Conntrack(None, capacity, seed=K.SEED + capacity, max_batch=257) as ct:
        model = R.Model(capacity)
        K.random_script(rng, model, R.HostRunner(ct), keys, 50 if capacity == 1024 else 80, SIZES)
        live, tombs, slots = ct.count()
        assert slots == max(2, 2 * capacity) and live == len(model.conns) <= capacity


def test_slot_count_and_home():
    for capacity, slots in ((1, 2), (2, 4), (3, 8), (4, 8), (1024, 2048), (1025, 4096)):
        with F.Conntrack(None, capacity, max_batch=1) as ct:
            assert ct.count() == (0, 0, slots)
    k = K.udp(7)
    with F.Conntrack(None, 1024, seed=1, max_batch=1) as a, F.Conntrack(None, 1024, seed=2, max_batch=1) as b, \
            F.Conntrack(None, 1024, seed=1, max_batch=1) as c:
        homes = [[t.home(K.udp(p)) for p in range(64)] for t in (a, b, c)]
        assert homes[0] == homes[2] != homes[1]  # the seed keys the hash
        assert len(set(homes[0])) > 48  # and it spreads
        a.add_host(k, [1], 5)
        assert a.entries()[R.keys_of(k)[0]][3] == a.home(k)


def test_argument_checks():
    lib = L.lib()
    h = C.c_void_p()
    for bad in ((0, 1), (L.CT_MAX_CAPACITY + 1, 1), (4, 0)):
        assert lib.neb_conntrack_create(None, bad[0], 0, 1, 1, 1, bad[1], C.byref(h)) == L.ERR_INVALID
    assert lib.neb_conntrack_destroy(None) == L.ERR_INVALID
    with F.Conntrack(None, 4, max_batch=2) as ct:
        fw = K.universe(3)
        st = np.zeros(3, np.int32)
        with pytest.raises(L.NebError):  # n > max_batch
            ct.lookup_host(fw, st, 0)
        with pytest.raises(L.NebError):
            ct.add_host(fw, [0, 0, 0], 0)
        with pytest.raises(L.NebError):
            ct.evict_host(fw, 0)
        # n == 0: NEB_OK, nothing written
        counts = np.full(4, 0xEE, np.uint32)
        assert lib.neb_conntrack_lookup_batch_host(ct.handle, None, None, 0, 0, None, None, None, None, 0,
                                                   counts.ctypes.data_as(C.c_void_p)) == L.OK
        assert (counts == 0xEE).all()
        assert lib.neb_conntrack_add_batch_host(ct.handle, None, None, 0, 0, None) == L.OK
        assert lib.neb_conntrack_evict_batch_host(ct.handle, None, 0, 0, 0, None) == L.OK
        # a host-only table given to a device call
        assert lib.neb_conntrack_lookup_batch(None, ct.handle, None, None, 0, 0, None, None, None, None, 0, None, None) == L.ERR_INVALID
        assert lib.neb_conntrack_add_batch(None, ct.handle, None, None, 0, 0, None, None) == L.ERR_INVALID
        assert lib.neb_conntrack_evict_batch(None, ct.handle, None, 0, 0, 0, None, None) == L.ERR_INVALID
        out = np.zeros(4, L.CT_SLOT_DTYPE)
        assert lib.neb_conntrack_dump(ct.handle, out.ctypes.data_as(C.c_void_p), 4) == L.ERR_INVALID  # not the slot count


def test_host_forms_take_unaligned_records():
    """The host forms align nothing: records at odd addresses."""
    fw = K.universe(5)
    raw = np.zeros(1 + fw.nbytes, np.uint8)
    raw[1:] = fw.view(np.uint8)
    odd = raw[1:].view(L.FW_PACKET_DTYPE)
    assert odd.ctypes.data % 2 == 1
    with F.Conntrack(None, 8, max_batch=8) as ct:
        lib = L.lib()
        res = np.zeros(1 + 5 * 8, np.uint8)
        inc = np.ones(5, np.uint8)
        assert lib.neb_conntrack_add_batch_host(ct.handle, odd.ctypes.data_as(C.c_void_p), inc.ctypes.data_as(C.c_void_p), 5, 1,
                                                C.c_void_p(res.ctypes.data + 1)) == L.OK
        assert [int(c) for c in res[1:].view(L.CT_RESULT_DTYPE)["code"]] == [L.CT_NEW] * 5
        v, work, counts = ct.lookup_host(fw, np.zeros(5, np.int32), 2)
        assert list(v) == [L.CT_HIT] * 5 and list(counts) == [5, 0, 0, 0]
