"""numpy restatement of the prefix cache's keys: the device digest of a 64-row block (include/vita_hip.h vh_hash_row_blocks) and the
host chain over it (vita_amd/serving.py chain_keys), written from the header's definition, not from the kernel."""
import hashlib

import numpy as np

GOLD = 0x9E3779B9
ROOT_KEY = hashlib.blake2b(b"vita_amd prefix cache v1", digest_size=16).digest()


def fmix32(h):
    """MurmurHash3's 32-bit finaliser on a uint32 array (arithmetic modulo 2^32)."""
    h = np.asarray(h, dtype=np.uint32).copy()
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def block_digest(block):
    """block: fp32 [64, cols] -> uint32 [4]"""
    words = np.ascontiguousarray(block, dtype=np.float32).view(np.uint32).reshape(-1)
    i = np.arange(words.size, dtype=np.uint64)
    out = np.zeros(4, dtype=np.uint32)
    with np.errstate(over="ignore"):
        for j in range(4):
            key = fmix32(((4 * i + j + GOLD) & 0xFFFFFFFF).astype(np.uint32))
            lane = int(fmix32(words ^ key).astype(np.uint64).sum() & 0xFFFFFFFF)
            out[j] = fmix32(np.array([(lane + (j + 1) * GOLD) & 0xFFFFFFFF], dtype=np.uint32))[0]
    return out


def digests(x):
    """x: fp32 [rows, cols] -> uint32 [rows // 64, 4]; a trailing partial block gets nothing."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0] // 64
    return np.stack([block_digest(x[64 * b:64 * b + 64]) for b in range(n)]) if n else np.zeros((0, 4), dtype=np.uint32)


def digest_bytes(x):
    """the digests as the 16-byte strings the chain takes (four little-endian words)."""
    return [d.astype("<u4").tobytes() for d in digests(x)]


def chain(dig_bytes, cols, parent=ROOT_KEY):
    keys = []
    for d in dig_bytes:
        parent = hashlib.blake2b(parent + d + int(cols).to_bytes(8, "little"), digest_size=16).digest()
        keys.append(parent)
    return keys


def keys(x):
    return chain(digest_bytes(x), np.asarray(x).shape[1])
