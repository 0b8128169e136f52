"""ctypes binding of libnebula_aead.so (the C ABI in include/nebula_aead.h).

The product path has exactly one implementation: the gfx950 kernels behind this library. If the
library is missing or does not load, every entry point raises — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# NEB_LIB_PATH selects an alternative build of the same library (e.g. an ablation build in tools/).
LIB_PATH = os.environ.get("NEB_LIB_PATH") or os.path.join(PKG_DIR, "libnebula_aead.so")

ALG_AESGCM = 1
ALG_CHACHAPOLY = 2

OK = 0
ERR_INVALID = -1
ERR_AUTH = -2
ERR_EXHAUSTED = -3
ERR_NO_CIPHER = -4
ERR_SHORT_BUFFER = -5
ERR_HIP = -6
ERR_NO_DEVICE = -7
ERR_NO_KEY_SLOT = -8

STATUS_OK = 0
STATUS_AUTH_FAILED = 1
STATUS_EXHAUSTED = 2
STATUS_BAD_KEY = 3
STATUS_REPLAY = 4
STATUS_INVALID = 5
STATUS_NO_SPACE = 6
STATUS_NOT_MESSAGE = 7
STATUS_NOT_FORWARDED = 8  # relay forwarding: not a verified Message/Relay packet, or no route
STATUS_NOT_RELAYED = 9  # neb_rx_open_via_batch's inner_status: not a verified terminal relay packet
STATUS_TX_DROPPED = 10  # neb_tx_resolve_batch: a gate dropped the read (FW_GATE_* says which)
STATUS_NO_ROUTE = 11  # neb_tx_resolve_batch: not in an own network and no route
STATUS_NO_TUNNEL = 12  # neb_tx_resolve_batch: no host entry yet, the caller handshakes
STATUS_RX_BAD_REMOTE = 13  # neb_rx_inner_batch: ErrInvalidRemoteIP
STATUS_RX_PEER_REJECTED = 14  # neb_rx_inner_batch: ErrPeerRejected
STATUS_RX_BAD_LOCAL = 15  # neb_rx_inner_batch: ErrInvalidLocalIP
STATUS_UNROUTABLE = 16  # neb_tx_send_plan: the socket cannot address the destination
STATUS_NOT_SENT = 17  # neb_tx_send_plan: wire_status != OK, never committed to the SendBatch
STATUS_FW_HELD = 18  # neb_conntrack_lookup_batch: held for the caller's rules (not an established flow)

OVERHEAD = 16
HEADER_LEN = 16
REJECT_HEADROOM = 1 << 40
REJECT_AFTER_MESSAGES = (1 << 64) - 1 - REJECT_HEADROOM
KEYS_MIXED = 0xFFFFFFFF
# neb_set_knob (include/nebula_aead.h)
KNOB_HOST_MODE, KNOB_SUB_BINS_FROM, KNOB_SINGLE_MAX_GRID, KNOB_RX_STRICT, KNOB_TILE_BINS_FROM = 0, 1, 2, 3, 4
KNOB_SMALL_BATCH, KNOB_FRONT_GROUPS = 5, 6
KNOB_COALESCE_HASH_BITS = 7  # the device coalescer's flow hash keeps this many bits (tests: collisions)
RELAY_NONE = 0xFFFFFFFF  # neb_relay_route.tunnel: do not forward (neb_tx_seal_via_batch: sent directly)
TX_WIRE_VIA = 1  # neb_tx_wire.reserved of a wire sent through a relay (neb_tx_seal_via_batch)
VIA_TERMINAL = 1  # neb_rx_via.flags: the outer header's relay is a TerminalType (the inner packet is ours)
RX_OWN_SOURCE = 0x80000000  # or-ed into neb_rx_packet.len: outside.go:66-74 refused the datagram

# neb_desc (include/nebula_aead.h)
DESC_DTYPE = np.dtype(
    [("src_off", "<u8"), ("dst_off", "<u8"), ("aad_off", "<u8"), ("counter", "<u8"),
     ("len", "<u4"), ("aad_len", "<u4"), ("key_id", "<u4"), ("flags", "<u4")]
)
assert DESC_DTYPE.itemsize == 48
# neb_rx_packet (include/nebula_aead.h): one received wire packet and its tunnel
RX_PACKET_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("key_id", "<u4")])
assert RX_PACKET_DTYPE.itemsize == 16
# neb_relay_route (include/nebula_aead.h): where a relayed packet goes (RELAY_NONE: nowhere)
RELAY_ROUTE_DTYPE = np.dtype([("tunnel", "<u4"), ("remote_index", "<u4")])
assert RELAY_ROUTE_DTYPE.itemsize == 8
# neb_rx_via (include/nebula_aead.h): the caller's lookups for the packet inside a relay packet
RX_VIA_DTYPE = np.dtype([("key_id", "<u4"), ("flags", "<u4")])
assert RX_VIA_DTYPE.itemsize == 8
# neb_index_table_* (include/nebula_aead.h): the hostmap's receive-side index lookups
INDEX_TUNNEL, INDEX_RELAY = 0, 1
INDEX_MAX_NETWORKS = 16
INDEX_KEY_DTYPE = np.dtype([("index", "<u4"), ("space", "<u4")])
INDEX_ENTRY_DTYPE = np.dtype([("index", "<u4"), ("space", "<u4"), ("key_id", "<u4"), ("flags", "<u4"),
                              ("tunnel", "<u4"), ("remote_index", "<u4")])
assert INDEX_ENTRY_DTYPE.itemsize == 24
CIDR_DTYPE = np.dtype([("addr", "u1", (16,)), ("family", "u1"), ("bits", "u1"), ("reserved", "u1", (2,))])
RX_SOURCE_DTYPE = np.dtype([("addr", "u1", (16,)), ("family", "u1"), ("reserved", "u1", (3,))])
assert CIDR_DTYPE.itemsize == 20 and RX_SOURCE_DTYPE.itemsize == 20

# neb_tx_table_* (include/nebula_aead.h): the TX-side lookups (VPN address -> tunnel, routes, ECMP)
TX_NO_TUNNEL = 0xFFFFFFFF
GATEWAY_NONE = 0xFFFFFFFF
ROUTE_MAX_GATEWAYS = 16
TX_DROP_LOCAL_BROADCAST, TX_DROP_MULTICAST = 1, 2
TX_KIND_HOST, TX_KIND_ROUTE = 0, 1
FW_FRAGMENT, FW_FRAG_ANY, FW_GATE_BROADCAST, FW_GATE_SELF, FW_GATE_MULTICAST = 0x01, 0x02, 0x04, 0x08, 0x10
FW_ROUTED, FW_ECMP_FALLBACK = 0x20, 0x40
TX_ADDR_DTYPE = np.dtype([("addr", "u1", (16,)), ("family", "u1"), ("reserved", "u1", (3,))])
TX_HOST_DTYPE = np.dtype([("addr", "u1", (16,)), ("family", "u1"), ("reserved", "u1", (3,)), ("tunnel", "<u4")])
GATEWAY_DTYPE = np.dtype([("addr", "u1", (16,)), ("family", "u1"), ("reserved", "u1", (3,)), ("weight", "<u4")])
ROUTE_DTYPE = np.dtype([("addr", "u1", (16,)), ("family", "u1"), ("bits", "u1"), ("reserved", "u1", (2,)),
                        ("ngateways", "<u4"), ("gateways", GATEWAY_DTYPE, (ROUTE_MAX_GATEWAYS,))])
FW_PACKET_DTYPE = np.dtype([("local_addr", "u1", (16,)), ("remote_addr", "u1", (16,)), ("local_port", "<u2"),
                            ("remote_port", "<u2"), ("protocol", "u1"), ("family", "u1"), ("flags", "u1"),
                            ("reserved", "u1"), ("ip_hdr_len", "<u2"), ("reserved2", "<u2"), ("gateway", "<u4")])
assert TX_ADDR_DTYPE.itemsize == 20 and TX_HOST_DTYPE.itemsize == 24
assert GATEWAY_DTYPE.itemsize == 24 and ROUTE_DTYPE.itemsize == 408 and FW_PACKET_DTYPE.itemsize == 48

# neb_peer_table_* (include/nebula_aead.h): every tunnel's certificate networks, the routable set
NET_VPN, NET_VPN_PEER, NET_UNSAFE = 1, 2, 3
RX_MAX_ROUTABLE = 32
PEER_NET_DTYPE = np.dtype([("tunnel", "<u4"), ("type", "<u4"), ("addr", "u1", (16,)), ("family", "u1"), ("bits", "u1"),
                           ("reserved", "u1", (2,))])
PEER_KEY_DTYPE = np.dtype([("tunnel", "<u4"), ("addr", "u1", (16,)), ("family", "u1"), ("bits", "u1"),
                           ("reserved", "u1", (2,))])
assert PEER_NET_DTYPE.itemsize == 28 and PEER_KEY_DTYPE.itemsize == 24

# neb_plain_packet (include/nebula_aead.h): one MultiCoalescer.Commit
PLAIN_PARSED, PLAIN_FRAG_ANY, PLAIN_SKIP = 1, 2, 4
PLAIN_PACKET_DTYPE = np.dtype([("off", "<u8"), ("epoch", "<u8"), ("counter", "<u8"), ("len", "<u4"),
                               ("ip_hdr_len", "<u2"), ("proto", "u1"), ("flags", "u1")])
assert PLAIN_PACKET_DTYPE.itemsize == 32
# neb_tun_write (include/nebula_aead.h): one write to the TUN with its virtio_net_hdr fields
TUN_WRITE_DTYPE = np.dtype([("out_off", "<u8"), ("len", "<u4"), ("first", "<u4"), ("nseg", "<u2"),
                            ("vnet_flags", "u1"), ("gso_type", "u1"), ("hdr_len", "<u2"), ("gso_size", "<u2"),
                            ("csum_start", "<u2"), ("csum_offset", "<u2"), ("lane", "u1"), ("reserved", "u1", (3,))])
assert TUN_WRITE_DTYPE.itemsize == 32
COALESCE_TCP, COALESCE_UDP = 1, 2
WRITE_NONE = 0xFFFFFFFF
VNET_F_NEEDS_CSUM, VNET_F_DATA_VALID = 1, 2

# neb_tx_send_plan (include/nebula_aead.h): sealed wires -> sendmmsg entries
SEND_NONE = 0xFFFFFFFF
SEND_MAX_BYTES = 65000
UDP_ADDR_DTYPE = np.dtype([("addr", "u1", (16,)), ("port", "<u2"), ("family", "u1"), ("reserved", "u1")])
SEND_IOV_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("wire", "<u4")])
SEND_ENTRY_DTYPE = np.dtype([("iov_first", "<u4"), ("niov", "<u2"), ("seg_size", "<u2"), ("dst", "<u4"),
                             ("bytes", "<u4")])
assert UDP_ADDR_DTYPE.itemsize == 20 and SEND_IOV_DTYPE.itemsize == 16 and SEND_ENTRY_DTYPE.itemsize == 16

# neb_rx_recv_plan (include/nebula_aead.h): recvmmsg entries with UDP_GRO -> wire packets
RECV_NONE = 0xFFFFFFFF
RECV_ENTRY_DTYPE = np.dtype([("off", "<u8"), ("len", "<u4"), ("seg_size", "<i4"), ("name", "u1", (28,)),
                             ("ctrl_len", "<u4")])
assert RECV_ENTRY_DTYPE.itemsize == 48

# neb_rx_report_batch (include/nebula_aead.h): a finished receive batch -> what the control plane acts on
REPORT_RELAYED = 1
REPORT_NMETRICS = 16
(METRIC_RX_HANDSHAKE, METRIC_RX_RECV_ERROR, METRIC_RX_LIGHTHOUSE, METRIC_RX_TEST_REQUEST, METRIC_RX_TEST_RESPONSE,
 METRIC_RX_CLOSE_TUNNEL, METRIC_RX_OTHER, METRIC_RX_INVALID, METRIC_OPENED, METRIC_OPENED_BYTES, METRIC_AUTH_FAILED,
 METRIC_REPLAY, METRIC_NO_TUNNEL) = range(13)
(WORK_HANDSHAKE, WORK_RECV_ERROR, WORK_NESTED_RELAY, WORK_SEND_RECV_ERROR, WORK_LIGHTHOUSE, WORK_TEST_REQUEST,
 WORK_CLOSE_TUNNEL, WORK_CONTROL) = range(1, 9)
RX_RUN_DTYPE = np.dtype([("bytes", "<u8"), ("key_id", "<u4"), ("packet", "<u4"), ("packets", "<u4"),
                         ("from", UDP_ADDR_DTYPE)])
RX_RELAY_USED_DTYPE = np.dtype([("index", "<u4"), ("packets", "<u4")])
RX_WORK_DTYPE = np.dtype([("packet", "<u4"), ("kind", "<u4")])
assert RX_RUN_DTYPE.itemsize == 40 and RX_RELAY_USED_DTYPE.itemsize == 8 and RX_WORK_DTYPE.itemsize == 8

# neb_conntrack_* (include/nebula_aead.h): firewall.Conntrack.Conns for TX and RX batches
CT_NONE, CT_HIT, CT_MISS, CT_STALE, CT_INCOMING = 0, 1, 2, 3, 0x80
CT_NEW, CT_EXISTING, CT_DUP, CT_FULL = 1, 2, 3, 4
CT_NO_SLOT = 0xFFFFFFFF
CT_MAX_CAPACITY = 1 << 22
CT_WORK_DTYPE = np.dtype([("packet", "<u4"), ("verdict", "<u4"), ("fw", FW_PACKET_DTYPE), ("reserved", "u1", (8,))])
CT_RESULT_DTYPE = np.dtype([("code", "<u4"), ("slot", "<u4")])
# one slot of the image (csrc/conntrack_core.hpp), as neb_conntrack_dump gives it
CT_SLOT_DTYPE = np.dtype([("state", "<u8"), ("key", "<u8", (5,)), ("expires", "<u8"), ("meta", "<u8")])
CT_STATE_EMPTY, CT_STATE_TOMB, CT_STATE_KIND, CT_STATE_CLAIMED, CT_STATE_SETTLED = 0, 1, 3 << 62, 2 << 62, 3 << 62
assert CT_WORK_DTYPE.itemsize == 64 and CT_RESULT_DTYPE.itemsize == 8 and CT_SLOT_DTYPE.itemsize == 64

# Every symbol include/nebula_aead.h declares, with (restype, argtypes).
_vp, _u8p, _sz, _u32, _u64, _i = C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64, C.c_int
SIGNATURES = {
    "neb_engine_create": (_i, [_i, _u32, C.POINTER(_vp)]),
    "neb_engine_destroy": (_i, [_vp]),
    "neb_engine_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_u32), C.POINTER(_u32)]),
    "neb_strerror": (C.c_char_p, [_i]),
    "neb_last_error": (C.c_char_p, []),
    "neb_build_id": (C.c_char_p, []),
    "neb_time_next_kernel": (_i, [_vp, _vp]),
    "neb_time_last_kernel": (C.c_char_p, []),
    "neb_set_knob": (_i, [_i, C.c_int64]),
    "neb_get_knob": (C.c_int64, [_i]),
    "neb_cipher_create": (_i, [_vp, _i, _u8p, C.POINTER(_vp)]),
    "neb_cipher_create_batch": (_i, [_vp, _i, _u8p, _u32, _vp]),
    "neb_cipher_create_multi": (_i, [_vp, _u32, _i, _u8p, _vp]),
    "neb_engine_stats": (_i, [_vp, _vp]),
    "neb_engine_pkt_combined": (_i, [_vp, _vp]),
    "neb_engine_pkt_launch": (_i, [_vp, _i, _vp, _u32, _vp]),
    "neb_cipher_destroy": (_i, [_vp]),
    "neb_cipher_key_id": (_u32, [_vp]),
    "neb_cipher_alg": (_i, [_vp]),
    "neb_cipher_name": (C.c_char_p, [_i]),
    "neb_overhead": (_i, [_vp]),
    "neb_encrypt_danger": (_i, [_vp, _u8p, _sz, _sz, _u8p, _sz, _u8p, _sz, _u64, _u8p, C.POINTER(_sz)]),
    "neb_decrypt_danger": (_i, [_vp, _u8p, _sz, _sz, _u8p, _sz, _u8p, _sz, _u64, _u8p, C.POINTER(_sz)]),
    "neb_seal_batch": (_i, [_vp, _i, _vp, _u32, _vp, _vp, _u32, _vp]),
    "neb_open_batch": (_i, [_vp, _i, _vp, _u32, _vp, _vp, _u32, _vp]),
    "neb_seal_batch_host": (_i, [_vp, _i, _vp, _u32, _vp, _sz, _vp, _u32]),
    "neb_open_batch_host": (_i, [_vp, _i, _vp, _u32, _vp, _sz, _vp, _u32]),
    "neb_host_alloc": (_i, [_sz, C.POINTER(_vp)]),
    "neb_host_free": (_i, [_vp]),
    "neb_header_encode": (None, [_u8p, C.c_uint8, C.c_uint8, C.c_uint8, _u32, _u64]),
    "neb_header_parse": (_i, [_u8p, _sz, _u8p, _u8p, _u8p, C.POINTER(C.c_uint16), C.POINTER(_u32),
                              C.POINTER(_u64)]),
    "neb_window_create": (_i, [_u64, C.POINTER(_vp)]),
    "neb_window_destroy": (_i, [_vp]),
    "neb_window_check": (_i, [_vp, _u64]),
    "neb_window_update": (_i, [_vp, _u64]),
    "neb_window_state": (_i, [_vp, C.POINTER(_u64), C.POINTER(C.c_int64)]),
    "neb_window_slot": (_i, [_vp, _u64]),
    "neb_window_reset_counters": (_i, [_vp]),
    "neb_rx_open_batch_host": (_i, [_vp, _i, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _u32]),
    "neb_dwindows_create": (_i, [_vp, _u32, _u64, _vp]),
    "neb_dwindows_destroy": (_i, [_vp]),
    "neb_dwindows_load": (_i, [_vp, _u32, _vp]),
    "neb_dwindows_store": (_i, [_vp, _u32, _vp]),
    "neb_dwindows_set_spin_limit": (_i, [_vp, _u32]),
    "neb_rx_open_batch": (_i, [_vp, _i, _vp, _vp, _u32, _vp, _vp, _u32, _vp]),
    "neb_tx_seal_batch": (_i, [_vp, _i, _vp, _u32, _vp, _u32, _vp, _vp, _sz, _vp, _vp, _u32, _vp, _vp, _u32, _vp]),
    "neb_tx_seal_batch_host": (_i, [_vp, _i, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _vp, _u32, _vp, _vp,
                                    _u32]),
    "neb_tx_seal_via_batch": (_i, [_vp, _i, _vp, _u32, _vp, _vp, _u32, _vp, _vp, _sz, _vp, _vp, _u32, _vp, _vp, _u32,
                                   _vp]),
    "neb_tx_seal_via_batch_host": (_i, [_vp, _i, _vp, _u32, _vp, _vp, _u32, _vp, _sz, _vp, _sz, _vp, _vp, _u32, _vp,
                                        _vp, _u32]),
    "neb_rx_open_wire_batch_host": (_i, [_vp, _i, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _u32]),
    "neb_rx_open_wire_batch": (_i, [_vp, _i, _vp, _vp, _u32, _vp, _vp, _u32, _vp]),
    "neb_relay_forward_batch": (_i, [_vp, _i, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _vp, _u32, _vp]),
    "neb_relay_forward_batch_host": (_i, [_vp, _i, _vp, _u32, _vp, _vp, _u32, _vp, _u32, _vp, _sz, _vp, _vp, _u32]),
    "neb_rx_open_via_batch": (_i, [_vp, _i, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp, _u32, _u32, _vp]),
    "neb_rx_open_via_batch_host": (_i, [_vp, _i, _vp, _u32, _vp, _vp, _u32, _vp, _sz, _vp, _vp, _vp, _u32, _u32]),
    "neb_rx_via_unwrap_host": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp, _vp]),
    "neb_tx_send_plan": (_i, [_vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp,
                              _vp, _vp, _vp]),
    "neb_tx_send_plan_host": (_i, [_vp, _vp, _u32, _vp, _u32, _vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp,
                                   _vp]),
    "neb_rx_coalesce_batch": (_i, [_vp, _vp, _u32, _vp, _vp, _sz, _vp, _u32, _vp, _vp, _vp, _u32, _vp]),
    "neb_rx_coalesce_batch_host": (_i, [_vp, _u32, _vp, _sz, _vp, _sz, _vp, _u32, _vp, _vp, _vp, _u32]),
    "neb_rx_plain_from_wire": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp]),
    "neb_rx_plain_from_wire_host": (_i, [_vp, _vp, _vp, _u32, _u32, _vp, _sz, _vp]),
    "neb_index_table_create": (_i, [_vp, _u32, C.POINTER(_vp)]),
    "neb_index_table_destroy": (_i, [_vp]),
    "neb_index_table_update": (_i, [_vp, _vp, _u32, _vp, _u32, _vp]),
    "neb_index_table_set_own_networks": (_i, [_vp, _vp, _u32, _vp]),
    "neb_index_table_count": (_i, [_vp, C.POINTER(_u32)]),
    "neb_index_table_probe": (_i, [_vp, _u32, _u32, C.POINTER(_u32)]),
    "neb_rx_resolve_batch": (_i, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "neb_rx_resolve_batch_host": (_i, [_vp, _vp, _vp, _u32, _vp, _sz, _vp, _vp]),
    "neb_rx_recv_plan": (_i, [_vp, _vp, _u32, _vp, _u32, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "neb_rx_recv_plan_host": (_i, [_vp, _u32, _vp, _u32, _u32, _vp, _vp, _vp, _u32, _vp, _vp, _vp]),
    "neb_rx_report_batch": (_i, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "neb_rx_report_batch_host": (_i, [_vp, _vp, _u32, _vp, _sz, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "neb_tx_table_create": (_i, [_vp, _u32, _u32, _u32, C.POINTER(_vp)]),
    "neb_tx_table_destroy": (_i, [_vp]),
    "neb_tx_table_update_hosts": (_i, [_vp, _vp, _u32, _vp, _u32, _vp]),
    "neb_tx_table_set_routes": (_i, [_vp, _vp, _u32, _vp]),
    "neb_tx_table_set_own": (_i, [_vp, _vp, _u32, _u32]),
    "neb_tx_table_count": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "neb_tx_table_probe": (_i, [_vp, _u32, _vp, C.POINTER(_u32)]),
    "neb_tx_resolve_batch": (_i, [_vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "neb_tx_resolve_batch_host": (_i, [_vp, _vp, _u32, _vp, _sz, _vp, _vp]),
    "neb_peer_table_create": (_i, [_vp, _u32, C.POINTER(_vp)]),
    "neb_peer_table_destroy": (_i, [_vp]),
    "neb_peer_table_update": (_i, [_vp, _vp, _u32, _vp, _u32, _vp]),
    "neb_peer_table_set_routable": (_i, [_vp, _vp, _u32]),
    "neb_peer_table_count": (_i, [_vp, C.POINTER(_u32)]),
    "neb_peer_table_probe": (_i, [_vp, _vp, C.POINTER(_u32)]),
    "neb_rx_inner_batch": (_i, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "neb_rx_inner_batch_host": (_i, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _sz, _vp, _vp, _vp]),
    "neb_conntrack_create": (_i, [_vp, _u32, _u64, _u64, _u64, _u64, _u32, C.POINTER(_vp)]),
    "neb_conntrack_destroy": (_i, [_vp]),
    "neb_conntrack_set_rules_version": (_i, [_vp, C.c_uint16]),
    "neb_conntrack_lookup_batch": (_i, [_vp, _vp, _vp, _vp, _u32, _u64, _vp, _vp, _vp, _vp, _u32, _vp, _vp]),
    "neb_conntrack_lookup_batch_host": (_i, [_vp, _vp, _vp, _u32, _u64, _vp, _vp, _vp, _vp, _u32, _vp]),
    "neb_conntrack_add_batch": (_i, [_vp, _vp, _vp, _vp, _u32, _u64, _vp, _vp]),
    "neb_conntrack_add_batch_host": (_i, [_vp, _vp, _vp, _u32, _u64, _vp]),
    "neb_conntrack_evict_batch": (_i, [_vp, _vp, _vp, _u32, _u64, _i, _vp, _vp]),
    "neb_conntrack_evict_batch_host": (_i, [_vp, _vp, _u32, _u64, _i, _vp]),
    "neb_conntrack_compact": (_i, [_vp, _vp]),
    "neb_conntrack_count": (_i, [_vp, C.POINTER(_u64)]),
    "neb_conntrack_home": (_i, [_vp, _vp, C.POINTER(_u32)]),
    "neb_conntrack_dump": (_i, [_vp, _vp, _u32]),
    "neb_seal_batch_host_multi": (_i, [_vp, _u32, _i, _vp, _u32, _vp, _sz, _vp, _u32]),
    "neb_open_batch_host_multi": (_i, [_vp, _u32, _i, _vp, _u32, _vp, _sz, _vp, _u32]),
    "neb_seal_batch_sharded": (_i, [_i, _vp, _u32, _u32]),
    "neb_open_batch_sharded": (_i, [_i, _vp, _u32, _u32]),
    "neb_queue_create": (_i, [_vp, _i, _i, _vp, C.POINTER(_vp)]),
    "neb_queue_destroy": (_i, [_vp]),
    "neb_queue_submit": (_i, [_vp, _vp, _u32, _vp, _sz, _vp]),
    "neb_queue_flush": (_i, [_vp]),
    "neb_queue_stats": (_i, [_vp, _vp]),
    "neb_queue_phases": (_i, [_vp, _vp]),
}


class Shard(C.Structure):
    """neb_shard (include/nebula_aead.h): one engine's device-resident part of a sharded batch."""
    _fields_ = [("e", C.c_void_p), ("d_desc", C.c_void_p), ("n", C.c_uint32), ("d_arena", C.c_void_p),
                ("d_status", C.c_void_p), ("stream", C.c_void_p)]


class PktReq(C.Structure):
    """neb_pkt_req (include/nebula_aead.h): one request of neb_engine_pkt_launch."""
    _fields_ = [("key_id", C.c_uint32), ("reserved", C.c_uint32), ("counter", C.c_uint64), ("ad", C.c_void_p),
                ("ad_len", C.c_size_t), ("in_", C.c_void_p), ("in_len", C.c_size_t), ("out", C.c_void_p)]


PKT_COMB_MAX = 32  # requests of one combined per-packet launch


class QueueConfig(C.Structure):
    """neb_queue_config (include/nebula_aead.h)."""
    _fields_ = [("max_packets", C.c_uint32), ("max_delay_us", C.c_uint32), ("arena_bytes", C.c_uint64),
                ("depth", C.c_uint32), ("reserved", C.c_uint32)]

_lib = None


class NebError(RuntimeError):
    def __init__(self, rc: int, what: str = ""):
        self.rc = rc
        msg = strerror(rc) if _lib is not None else str(rc)
        if _lib is not None and rc in (ERR_HIP, ERR_NO_DEVICE):
            detail = _lib.neb_last_error().decode()
            if detail:
                msg += f" [{detail}]"
        super().__init__(f"{what}: {msg} ({rc})" if what else f"{msg} ({rc})")


def build() -> None:
    """Compile libnebula_aead.so in-tree (hipcc --offload-arch=gfx950)."""
    subprocess.run(["make", "-s", "-C", PKG_DIR], check=True)


def _pin_hip_runtime() -> None:
    """Load PyTorch's HIP runtime before ours when torch is installed.

    torch-ROCm ships its own libamdhip64.so.7 (same SONAME as /opt/rocm's). Whichever is loaded
    first serves the whole process, and torch cannot initialise the GPU on a runtime it did not
    bring. Importing torch first makes every HIP call in the process, ours included, go through
    one runtime, so torch tensors, streams and events interoperate with the engine.
    """
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def lib():
    global _lib
    if _lib is None:
        _pin_hip_runtime()
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with `make -C {PKG_DIR}` "
                               "(nebula_amd has no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("NEB_LIB_PATH") and not hasattr(L, name):
                continue  # an older A/B build (tools/ab.sh) may predate some entry points
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def strerror(rc: int) -> str:
    return lib().neb_strerror(rc).decode()


def check(rc: int, what: str = "") -> None:
    if rc != OK:
        raise NebError(rc, what)


class knob:
    """`with knob(KNOB_X, v):` sets a process-wide knob (neb_set_knob) and restores it after."""

    def __init__(self, k: int, value: int):
        self.k, self.value = k, value

    def __enter__(self):
        self.old = lib().neb_get_knob(self.k)
        check(lib().neb_set_knob(self.k, self.value), "neb_set_knob")
        return self

    def __exit__(self, *exc):
        lib().neb_set_knob(self.k, self.old)
