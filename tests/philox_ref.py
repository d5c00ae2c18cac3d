"""Host restatement of the library's noise generator (frido_amd/csrc/philox.h: Philox4x32-10 + Box-Muller), for the tests.

Integer part: plain unsigned arithmetic on numpy uint64 arrays (a 32 x 32 bit product fits 64 bits), vectorised over any leading shape.
Counter {grp, draw, sample lo, sample hi ^ (stream << 20)}, key {seed lo, seed hi}.  Uniforms: formed in float32 exactly as the header
forms them -- (float(c) + 1) * 2^-32 for the radius words 0 and 2 (so the logarithm never sees 0; a word of 2^32 - 1 gives exactly 1),
float(c) * 2^-32 for the angle words 1 and 3, and the fp32 product 6.2831855f * u.  log, sqrt, sin and cos are then evaluated in float64 ON
those fp32 inputs, so what separates a kernel from this reference is the error of the device's logf / sqrtf / sincosf and one product
rounding: a few fp32 ulp.  A mistake in the integer part (multiplier, round count, counter layout, key schedule) moves values by O(1).

`rounds` and `swap_grp_draw` exist to state WRONG generators (nine rounds; grp and draw exchanged in the counter), which the tests use to
show that their bounds tell the right generator from a near miss.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)      # round multipliers (Salmon et al., SC'11, table 2)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)      # Weyl key increments
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
TWO_PI_F32 = np.float32(6.2831855)
TWO_M32 = np.float32(2.0 ** -32)
VMAX = float(np.sqrt(64.0 * np.log(2.0)))                  # |v| <= sqrt(-2 ln 2^-32) = 6.6604: the smallest radius uniform is 2^-32


def philox4x32(ctr, key, rounds=10):
    """ctr [..., 4], key [..., 2] (broadcastable leading shapes; values < 2^32) -> uint64 array [..., 4] of 32-bit words."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    key = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (ctr[..., i] for i in range(4))
    k0, k1 = key[..., 0], key[..., 1]
    for _ in range(rounds):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def counter(seed, sample, draw, stream, grp, swap_grp_draw=False):
    """(ctr [..., 4], key [2]) of randn4(seed, sample, draw, stream, grp); sample / draw / grp may be integer arrays (broadcast)."""
    sample = np.asarray(sample, dtype=np.int64).astype(np.uint64)              # int64 -> its two's-complement bits
    grp = np.asarray(grp, dtype=np.int64).astype(np.uint64) & MASK
    draw = np.asarray(draw, dtype=np.int64).astype(np.uint64) & MASK
    hi = (sample >> S32) ^ np.uint64((int(stream) << 20) & 0xFFFFFFFF)
    w0, w1 = (draw, grp) if swap_grp_draw else (grp, draw)
    ctr = np.stack(np.broadcast_arrays(w0, w1, sample & MASK, hi), axis=-1)
    seed = int(seed) & (2 ** 64 - 1)
    return ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)


def box_muller(words):
    """uint64 words [..., 4] -> float64 normals [..., 4] = {r0 cos, r0 sin, r1 cos, r1 sin}: fp32 uniforms, float64 transcendentals."""
    f = np.asarray(words, dtype=np.uint64).astype(np.uint32).astype(np.float32)      # (float)c: round to nearest even
    one = np.float32(1.0)
    u_r = np.minimum((f[..., 0::2] + one) * TWO_M32, one)                             # words 0, 2 -> (0, 1]
    ang = TWO_PI_F32 * (f[..., 1::2] * TWO_M32)                                       # words 1, 3 -> [0, 2 pi], fp32 product
    assert u_r.dtype == np.float32 and ang.dtype == np.float32
    r = np.sqrt(-2.0 * np.log(u_r.astype(np.float64)))
    a = ang.astype(np.float64)
    out = np.empty(f.shape, dtype=np.float64)
    out[..., 0::2] = r * np.cos(a)
    out[..., 1::2] = r * np.sin(a)
    return out


def randn4(seed, sample, draw, stream, grp, rounds=10, swap_grp_draw=False):
    """float64 [..., 4]: the four normals of group `grp` of draw `draw` of global sample `sample`."""
    ctr, key = counter(seed, sample, draw, stream, grp, swap_grp_draw)
    return box_muller(philox4x32(ctr, key, rounds))


def randn_fill(seed, sample0, stream, per_sample, groups, **kw):
    """frido_randn's numbering: flat group g (4 floats) belongs to sample sample0 + g // (per_sample / 4), group g % (per_sample / 4),
    draw 0.  groups: integer array of flat group indices -> float64 [len(groups), 4]."""
    groups = np.asarray(groups, dtype=np.int64)
    gps = (int(per_sample) + 3) >> 2
    smp = groups // gps
    return randn4(seed, int(sample0) + smp, 0, stream, groups - smp * gps, **kw)


def sampler_noise(seed, sample0, stream, draw, B, HW, nch, **kw):
    """The draws inside the DDIM / PLMS update: pixel p of sample b takes groups p * ngrp + g, g < ngrp = ceil(nch / 4), of draw
    `draw` (= device step + coef_row_offset + 1); channel c is element c % 4 of group c // 4.  -> float64 [B, HW, nch]."""
    ngrp = (nch + 3) >> 2
    b = np.arange(B, dtype=np.int64)[:, None, None]
    p = np.arange(HW, dtype=np.int64)[None, :, None]
    g = np.arange(ngrp, dtype=np.int64)[None, None, :]
    v = randn4(seed, int(sample0) + b, draw, stream, p * ngrp + g, **kw)             # [B, HW, ngrp, 4]
    return v.reshape(B, HW, ngrp * 4)[..., :nch]
