"""The keep bits of the encoder's training dropout, restated on the CPU (numpy only, no GPU, no library).

csrc/ccr_dropout.hip writes the bits the layer kernels read; this module computes the same bits from (seed, stream, p, shape), so a
test or a user can rebuild any mask a training forward used (FusedBertEncoder.last_seed, stream ids in fused_bert.dropout_stream).

The generator is counter based.  One Philox4x32-10 call (multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85,
key = the 64-bit seed's low and high word) gives four 32-bit words = eight 16-bit lanes: low half of word 0, high half of word 0, low
half of word 1, ...  Lane j decides element 8 * group + j of its index row: keep iff lane >= thr = round(p * 65536).

  row-wise sites ([rows, dim], dim % 256 == 0, dim <= 2048: the kernels' contract):  counter = (row, column >> 3, stream, 0)
  attention sites:                              counter = (token row of the query, key >> 3, stream, head)

Packed layouts (uint32, bit 1 = keep): rows_bits [rows, dim / 32], bit i of word w <-> column 32 w + i; attention_bits -> keep_q
[T, H, W] (row = the query's token row, bit = key position) and keep_k [T, H, W] (row = the key's token row, bit = query position),
W = ceil(max_len / 32).  Bits of positions at or beyond a sequence's length are unspecified on the device; here they are zero."""
import math

import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) broadcastable to one shape, key: two ints -> uint32 array [..., 4]."""
    c = [np.asarray(x, dtype=np.uint64) & _LOW for x in np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) for v in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]                      # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> _32) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> _32) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def threshold(p):
    """thr = round(p * 65536) (halves up) of a dropout probability 0 <= p < 1; a lane keeps its element iff lane >= thr."""
    p = float(p)
    thr = int(math.floor(p * 65536.0 + 0.5)) if 0.0 <= p < 1.0 else 65536
    if thr >= 65536:
        raise ValueError(f"dropout probability {p!r}: 0 <= p and round(p * 65536) < 65536")
    return thr


def p_eff(p):
    """The probability actually used: thr / 65536 (0.100006 for p = 0.1)."""
    return threshold(p) / 65536.0


def inv_keep(p):
    """The scale of a kept element, 65536 / (65536 - thr) rounded to fp32 (what the kernels multiply by): E[keep * inv_keep] = 1 exactly
    for p_eff."""
    return float(np.float32(65536.0 / (65536 - threshold(p))))


def _seed_key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def _decisions(a, n, stream, d, seed, p):
    """bool [len(a), n]: keep decisions of elements 0 .. n - 1 of the index rows `a` (fourth counter word d, scalar or per row)."""
    a = np.asarray(a, dtype=np.uint64).reshape(-1)
    groups = (n + 7) // 8
    d = np.broadcast_to(np.asarray(d, dtype=np.uint64).reshape(-1, 1), (a.size, 1))
    out = philox4x32_10((a[:, None], np.arange(groups, dtype=np.uint64)[None, :], np.uint64(int(stream) & 0xFFFFFFFF), d), _seed_key(seed))
    lanes = np.stack([out & np.uint32(0xFFFF), out >> np.uint32(16)], axis=-1).reshape(a.size, groups * 8)   # word 0 low, word 0 high, ...
    return (lanes >= np.uint32(threshold(p)))[:, :n]


def pack_bits(mask):
    """bool [..., n] -> uint32 [..., ceil(n / 32)]: bit i of word w <-> element 32 w + i (missing elements: 0)."""
    mask = np.asarray(mask, dtype=bool)
    n = mask.shape[-1]
    words = (n + 31) // 32
    padded = np.zeros(mask.shape[:-1] + (words * 32,), dtype=np.uint64)
    padded[..., :n] = mask
    weights = np.uint64(1) << np.arange(32, dtype=np.uint64)
    return (padded.reshape(mask.shape[:-1] + (words, 32)) * weights).sum(axis=-1).astype(np.uint32)


def unpack_bits(bits, n):
    """uint32 [..., W] -> bool [..., n]."""
    bits = np.asarray(bits, dtype=np.uint32)
    out = (bits[..., :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return out.reshape(bits.shape[:-1] + (bits.shape[-1] * 32,))[..., :n].astype(bool)


def rows_mask(seed, stream, p, rows, dim):
    """bool [rows, dim]: the keep decisions of a row-wise site."""
    assert dim > 0 and dim % 256 == 0 and dim <= 2048, f"dim={dim}: a multiple of 256 up to 2048, as ccr_dropout_bits_rows takes it"
    return _decisions(np.arange(rows), dim, stream, 0, seed, p)


def rows_bits(seed, stream, p, rows, dim):
    """uint32 [rows, dim / 32]: what ccr_dropout_bits_rows writes."""
    return pack_bits(rows_mask(seed, stream, p, rows, dim))


def attention_mask(seed, stream, p, seq_start, seq_len, n_heads):
    """One bool array [n_heads, len, len] (query, key) per sequence: the keep decisions of an attention site."""
    out = []
    for start, n in zip(seq_start, seq_len):
        start, n = int(start), int(n)
        q = np.repeat(np.arange(start, start + n), n_heads)                      # (query, head) pairs, head fastest
        h = np.tile(np.arange(n_heads), n)
        m = _decisions(q, n, stream, h, seed, p) if n else np.zeros((0, 0), dtype=bool)
        out.append(m.reshape(n, n_heads, n).transpose(1, 0, 2))
    return out


def attention_bits(seed, stream, p, seq_start, seq_len, n_heads, max_len, n_tokens):
    """(keep_q, keep_k) uint32 [n_tokens, n_heads, W]: what ccr_dropout_bits_attention writes on the positions below each length
    (everything else is zero here)."""
    W = (int(max_len) + 31) // 32
    keep_q = np.zeros((n_tokens, n_heads, W), dtype=np.uint32)
    keep_k = np.zeros((n_tokens, n_heads, W), dtype=np.uint32)
    for start, n, m in zip(seq_start, seq_len, attention_mask(seed, stream, p, seq_start, seq_len, n_heads)):
        start, n = int(start), int(n)
        if n == 0:
            continue
        w = (n + 31) // 32
        keep_q[start:start + n, :, :w] = pack_bits(m.transpose(1, 0, 2))         # [query, head, key]
        keep_k[start:start + n, :, :w] = pack_bits(m.transpose(2, 0, 1))         # [key, head, query]
    return keep_q, keep_k
