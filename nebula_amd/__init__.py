"""nebula_amd — MI355X-native (gfx950) engine for Nebula's per-packet AEAD data plane.

Product path: include/nebula_aead.h (C ABI) -> libnebula_aead.so (hand-written HIP kernels for
AES-256-GCM and ChaCha20-Poly1305). The Python modules mirror the reference's noiseutil /
header surface on top of that ABI; they never compute a byte of ciphertext themselves.
"""
from . import _lib
from ._lib import (ALG_AESGCM, ALG_CHACHAPOLY, DESC_DTYPE, KEYS_MIXED, OVERHEAD, REJECT_AFTER_MESSAGES,
                   NebError, build)
from .noiseutil import (CipherAESGCM, CipherChaChaPoly, CipherState, CipherStateAESGCM, CipherStateChaChaPoly,
                        Engine, ErrMessageCounterExhausted, ErrNoCipher, ErrOpen, NewCipherState,
                        RejectAfterMessages, RejectHeadroom, Slice)
from .firewall import Conntrack
from .hostmap import IndexTable, PeerTable, TxTable
from .outside import MultiCoalescer, coalesce_batch_device, coalesce_batch_host, inner_device, inner_host, receive
from .relay import (relay_forward_batch, relay_forward_batch_device, rx_open_via_batch, rx_open_via_batch_device,
                    rx_via_unwrap)

__all__ = [
    "ALG_AESGCM", "ALG_CHACHAPOLY", "DESC_DTYPE", "KEYS_MIXED", "OVERHEAD", "REJECT_AFTER_MESSAGES",
    "NebError", "build", "CipherAESGCM", "CipherChaChaPoly", "CipherState", "CipherStateAESGCM",
    "CipherStateChaChaPoly", "Engine", "ErrMessageCounterExhausted", "ErrNoCipher", "ErrOpen",
    "NewCipherState", "RejectAfterMessages", "RejectHeadroom", "Slice", "_lib",
    "relay_forward_batch", "relay_forward_batch_device", "rx_open_via_batch", "rx_open_via_batch_device",
    "rx_via_unwrap", "IndexTable", "TxTable", "PeerTable", "inner_host", "inner_device",
    "MultiCoalescer", "coalesce_batch_host", "coalesce_batch_device", "receive", "Conntrack",
]
