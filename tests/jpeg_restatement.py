"""NumPy restatement of the device half of the JPEG decoder (csrc/jpeg_decode.hip): quantised coefficients in the
layout vnf_jpeg_entropy_decode writes -> (H,W,3) u8 RGB, with libjpeg's public baseline arithmetic (islow IDCT, fancy
upsampling, 16-bit fixed-point colour).  Independent of the kernels: whole-plane array arithmetic, no shared code.
Also a few-line DQT / SOF0 / DRI reader in Python, so that the probe's answers are checked against something that is not
the C++ under test, and the loader of tests/golden/jpeg_cases.npz (tools/make_jpeg_golden.py)."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GRAY, S444, S422, S420 = 0, 1, 2, 3
ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
          28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54,
          47, 55, 62, 63]


def _idct8(x, shift):
    """x: list of 8 int64 arrays (frequency 0..7) -> list of 8 (position 0..7), descaled by `shift` with rounding"""
    z2, z3 = x[2], x[6]
    z1 = (z2 + z3) * 4433
    tmp2 = z1 + z3 * (-15137)
    tmp3 = z1 + z2 * 6270
    tmp0 = (x[0] + x[4]) * 8192
    tmp1 = (x[0] - x[4]) * 8192
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = x[7], x[5], x[3], x[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * 9633
    tmp0, tmp1, tmp2, tmp3 = tmp0 * 2446, tmp1 * 16819, tmp2 * 25172, tmp3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    r = 1 << (shift - 1)
    out = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    return [(o + r) >> shift for o in out]


def idct_plane(coefs, quant, bw, bh):
    """coefs: (bh*bw*64,) int16 blocks in raster order; quant (64,) -> (bh*8, bw*8) u8 plane"""
    v = coefs.astype(np.int64).reshape(bh * bw, 8, 8) * quant.astype(np.int64).reshape(1, 8, 8)
    cols = _idct8([v[:, k, :] for k in range(8)], 11)            # pass 1: down the columns -> rows 0..7
    ws = np.stack(cols, axis=1)
    rows = _idct8([ws[:, :, k] for k in range(8)], 18)           # pass 2: along the rows
    px = np.stack(rows, axis=2)
    m = px & 1023                                                # range_limit[x & RANGE_MASK]
    m = np.where(m >= 512, m - 1024, m)
    px = np.clip(m + 128, 0, 255).astype(np.uint8)
    return px.reshape(bh, bw, 8, 8).transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)


def _h2(c, lo, hi, shift):
    """triangle filter along the last axis: out[2i] = (3c[i] + c[i-1] + lo) >> shift, out[2i+1] = (3c[i] + c[i+1] + hi)
    >> shift, edges replicated (which gives libjpeg's special first and last column)"""
    p = np.pad(c, ((0, 0), (1, 1)), mode="edge")
    out = np.empty((c.shape[0], c.shape[1] * 2), np.int64)
    out[:, 0::2] = (3 * p[:, 1:-1] + p[:, :-2] + lo) >> shift
    out[:, 1::2] = (3 * p[:, 1:-1] + p[:, 2:] + hi) >> shift
    return out


def upsample(plane, sampling, W, H):
    """real chroma samples of the padded plane -> (H, W) int64"""
    if sampling == S444:
        return plane[:H, :W].astype(np.int64)
    cw = (W + 1) // 2
    if sampling == S422:
        return _h2(plane[:H, :cw].astype(np.int64), 1, 2, 2)[:, :W]
    ch = (H + 1) // 2
    c = plane[:ch, :cw].astype(np.int64)
    p = np.pad(c, ((1, 1), (0, 0)), mode="edge")
    v = np.empty((ch * 2, cw), np.int64)
    v[0::2] = 3 * c + p[:-2]                                     # upper output row: far = the row above
    v[1::2] = 3 * c + p[2:]
    return _h2(v, 8, 7, 4)[:H, :W]


def ycc_to_rgb(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb - 128, cr - 128
    F = lambda x: int(x * 65536 + 0.5)
    r = y + ((F(1.402) * cr + 32768) >> 16)
    b = y + ((F(1.772) * cb + 32768) >> 16)
    g = y + ((-F(0.34414) * cb + 32768 - F(0.71414) * cr) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def coefs_to_rgb(coefs, quant, W, H, sampling, blocks_w, blocks_h):
    """coefs: (coef_count,) int16; quant (3,64) u8 natural order -> (H,W,3) u8"""
    planes, o = [], 0
    for c in range(1 if sampling == GRAY else 3):
        n = 64 * blocks_w[c] * blocks_h[c]
        planes.append(idct_plane(coefs[o:o + n], quant[c], blocks_w[c], blocks_h[c]))
        o += n
    y = planes[0][:H, :W]
    if sampling == GRAY:
        return np.repeat(y[:, :, None], 3, axis=2)
    return ycc_to_rgb(y, upsample(planes[1], sampling, W, H), upsample(planes[2], sampling, W, H))


def read_header(data):
    """-> dict(width, height, sof, comps=[(id, h, v, tq)], quant={tq: (64,) natural order}, dri, scan) from the marker
    segments in front of the first scan"""
    out = {"quant": {}, "dri": 0, "sof": None}
    p = 2
    while p + 4 <= len(data):
        assert data[p] == 0xFF
        m = data[p + 1]
        L = (data[p + 2] << 8) | data[p + 3]
        s = data[p + 4:p + 2 + L]
        if m == 0xDB:
            q = 0
            while q < len(s):
                assert s[q] >> 4 == 0
                t = np.zeros(64, np.uint8)
                t[ZIGZAG] = np.frombuffer(bytes(s[q + 1:q + 65]), np.uint8)
                out["quant"][s[q] & 15] = t
                q += 65
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            out["sof"] = m
            out["height"], out["width"] = (s[1] << 8) | s[2], (s[3] << 8) | s[4]
            out["comps"] = [(s[6 + 3 * c], s[7 + 3 * c] >> 4, s[7 + 3 * c] & 15, s[8 + 3 * c]) for c in range(s[5])]
        elif m == 0xDD:
            out["dri"] = (s[0] << 8) | s[1]
        elif m == 0xDA:
            out["scan"] = p + 2 + L                  # the first entropy-coded byte
            break
        p += 2 + L
    return out


_cases = None


def load_cases():
    """-> (list of dict(name, jpg: bytes, rgb: (H,W,3) u8 or None, + the generator's parameters), versions dict); read
    once, shared, never modified by the tests"""
    global _cases
    if _cases is None:
        z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
        meta = json.loads(bytes(z["meta"]).decode())
        cases = []
        for i, m in enumerate(meta["cases"]):
            c = dict(m)
            c["jpg"] = bytes(z["jpg_%d" % i])
            c["rgb"] = z["rgb_%d" % i] if ("rgb_%d" % i) in z.files else None
            if c["rgb"] is not None:
                c["rgb"].setflags(write=False)
            cases.append(c)
        _cases = (cases, meta["versions"])
    return _cases
