"""NumPy restatement of the device half of the JPEG frame encoder (csrc/jpeg_encode.hip) and of the frame overlay
(csrc/overlay.hip): what the kernels must compute, stated without them, so that the arithmetic is pinned on a machine
without a GPU.  The expected numbers are Pillow's: the quantised coefficients of the files it writes (read back through
vnf_jpeg_entropy_decode) and the pixels cli_utils.draw_boxes_on_image paints.

Encoder (libjpeg's baseline path, all integer): RGB -> YCbCr in 16-bit fixed point, chroma down-sampling with the
alternating bias, edge replication, the "islow" forward DCT (13-bit constants, 2 extra bits between the passes) on
samples - 128, quantisation by division with rounding half away from zero, and the dummy blocks that pad a plane to
whole MCUs (all zero but a DC copied from a neighbour's quantised DC).
"""
import io

import numpy as np

GRAY, S444, S422, S420 = 0, 1, 2, 3
FACTORS = {S444: (1, 1), S422: (2, 1), S420: (2, 2)}
PIL_SUBSAMPLING = {S444: 0, S422: 1, S420: 2}

SIZES = [(1, 1), (8, 8), (8, 24), (24, 8), (9, 17), (17, 9), (16, 16), (31, 33), (33, 47), (64, 48), (130, 70)]  # (W, H)
QUALITIES = [30, 75, 92, 100]

# ITU-T T.81 annex K.1 / K.2, natural order
LUMA_BASE = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
CHROMA_BASE = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)


def quant_tables(quality):
    """(2,64) u8: jpeg_quality_scaling + jpeg_add_quant_table (force_baseline) on the annex K tables"""
    q = int(quality)
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * scale + 50) // 100, 1, 255) for b in (LUMA_BASE, CHROMA_BASE)]).astype(np.uint8)


def make_frame(w, h, content, seed=0):
    """(h,w,3) u8: 'noise' uniform bytes, 'ramp' a smooth colour gradient"""
    if content == "noise":
        return np.random.default_rng(1000 * w + h + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    r = (x * 255) // max(1, w - 1)
    g = (y * 255) // max(1, h - 1)
    b = ((x + y + 7 * seed) * 255) // max(1, w + h - 2 + 7 * seed)
    return np.stack([r, g, b], axis=2).astype(np.uint8)


def pillow_jpeg(rgb, quality, sampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(rgb).save(buf, format="JPEG", quality=int(quality), subsampling=PIL_SUBSAMPLING[sampling])
    return buf.getvalue()


def geometry(w, h, sampling):
    """-> (hf, vf, blocks_w[3], blocks_h[3], coef_count) of the decoder's coefficient layout"""
    hf, vf = FACTORS[sampling]
    mx, my = -(-w // (8 * hf)), -(-h // (8 * vf))
    bw, bh = [mx * hf, mx, mx], [my * vf, my, my]
    return hf, vf, bw, bh, 64 * sum(a * b for a, b in zip(bw, bh))


def rgb_to_ycc(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _pad(a, rows, cols):
    return np.pad(a, ((0, rows - a.shape[0]), (0, cols - a.shape[1])), mode="edge")


def planes(rgb, sampling):
    """the three edge-replicated sample planes launch 1 writes: luma (hb*8, wb*8) over the REAL blocks only, chroma
    (chb*8, cwb*8)"""
    h, w = rgb.shape[:2]
    hf, vf = FACTORS[sampling]
    y, cb, cr = rgb_to_ycc(rgb)
    out = [_pad(y, -(-h // 8) * 8, -(-w // 8) * 8)]
    cw, ch = -(-w // hf), -(-h // vf)
    cwb, chb = -(-cw // 8), -(-ch // 8)
    for c in (cb, cr):
        full = _pad(c, ch * vf, cwb * 8 * hf)             # columns all the way, rows only to whole chroma samples
        if (hf, vf) == (1, 1):
            ds = full
        elif (hf, vf) == (2, 1):
            ds = (full[:, 0::2] + full[:, 1::2] + (np.arange(cwb * 8) & 1)[None, :]) >> 1
        else:
            ds = (full[0::2, 0::2] + full[0::2, 1::2] + full[1::2, 0::2] + full[1::2, 1::2] +
                  (1 + (np.arange(cwb * 8) & 1))[None, :]) >> 2
        out.append(_pad(ds, chb * 8, cwb * 8))            # the DOWN-SAMPLED last row goes on down
    return out


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first):
    """one pass of jfdctint.c over the last axis of d (..., 8)"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    sh = 11 if first else 15
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, sh)
    o[6] = _descale(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7] = _descale(t4 + z1 + z3, sh)
    o[5] = _descale(t5 + z2 + z4, sh)
    o[3] = _descale(t6 + z2 + z3, sh)
    o[1] = _descale(t7 + z1 + z4, sh)
    return np.stack(o, axis=-1)


def fdct_quant(plane, quant):
    """(R*8, C*8) samples -> (R, C, 64) quantised coefficients, natural order"""
    r, c = plane.shape[0] // 8, plane.shape[1] // 8
    blk = plane.reshape(r, 8, c, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    blk = _fdct_1d(blk, True)                                             # rows
    blk = _fdct_1d(blk.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)  # columns
    q8 = quant.astype(np.int64).reshape(8, 8) * 8
    mag = (np.abs(blk) + (q8 >> 1)) // q8
    return (np.sign(blk) * mag).reshape(r, c, 64)


def encode_coefs(rgb, quant2, sampling):
    """(H,W,3) u8, (2,64) tables -> the frame's coef_count int16 coefficients in vnf_jpeg_entropy_decode's layout"""
    h, w = rgb.shape[:2]
    hf, vf, bw, bh, count = geometry(w, h, sampling)
    pl = planes(rgb, sampling)
    out = []
    real = fdct_quant(pl[0], quant2[0])
    hb, wb = real.shape[:2]
    luma = np.zeros((bh[0], bw[0], 64), np.int64)
    luma[:hb, :wb] = real
    for by in range(bh[0]):
        for bx in range(bw[0]):
            if by < hb and bx < wb:
                continue
            if by >= hb:       # the MCU's bottom dummy row: the LAST block of the row above in this MCU, itself filled
                sx = min((bx // hf) * hf + hf - 1, wb - 1)
            else:
                sx = wb - 1
            luma[by, bx, 0] = real[min(by, hb - 1), sx, 0]
    out.append(luma.reshape(-1))
    for c in (1, 2):
        co = fdct_quant(pl[c], quant2[1])
        assert co.shape[:2] == (bh[c], bw[c])
        out.append(co.reshape(-1))
    res = np.concatenate(out)
    assert res.size == count
    return res.astype(np.int16)


# overlay -------------------------------------------------------------------------------------------------------------

def label_tile(name, fx, fy):
    """the coverage mask of a label as Pillow itself renders it at the sub-pixel offset (fx, fy): (th,tw) u8, cut to
    the rows and columns that hold ink (None: no ink) and the offset (ox, oy) of the cut inside the tile"""
    from PIL import Image, ImageDraw
    probe = ImageDraw.Draw(Image.new("L", (1, 1)))
    l, t, r, b = probe.textbbox((fx, fy), str(name))
    tw, th = max(1, int(np.ceil(r)) + 2), max(1, int(np.ceil(b)) + 2)
    im = Image.new("L", (tw, th), 0)
    ImageDraw.Draw(im).text((fx, fy), str(name), fill=255)
    a = np.asarray(im)
    ys, xs = np.nonzero(a)
    if ys.size == 0:
        return None, 0, 0
    y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
    return np.ascontiguousarray(a[y0:y1, x0:x1]), int(x0), int(y0)


def overlay(frame, boxes, names, colour=(0, 255, 0)):
    """what vnf_overlay_draw paints for jpeg_encode.overlay_ops(boxes, names) on one frame, in NumPy"""
    import math
    out = np.asarray(frame, np.uint8).copy()
    h, w = out.shape[:2]
    col = np.array(colour, np.int64)
    for box, name in zip(boxes, names):
        x0, y0, x1, y1 = (int(float(v)) for v in box[:4])
        if x1 >= x0 and y1 >= y0:
            yy, xx = np.mgrid[0:h, 0:w]
            inside = (xx >= x0) & (xx <= x1) & (yy >= y0) & (yy <= y1)
            hole = (xx >= x0 + 2) & (xx <= x1 - 2) & (yy >= y0 + 2) & (yy <= y1 - 2)
            out[inside & ~hole] = col
        ax, ay = float(box[2]), float(box[1])
        fx, ix = math.modf(ax)
        fy, iy = math.modf(ay)
        m, ox, oy = label_tile(name, fx, fy)
        if m is None:
            continue
        px, py = int(ix) + ox, int(iy) + oy
        for ty in range(m.shape[0]):
            for tx in range(m.shape[1]):
                x, y, a = px + tx, py + ty, int(m[ty, tx])
                if a and 0 <= x < w and 0 <= y < h:
                    v = out[y, x].astype(np.int64) * (255 - a) + col * a + 128
                    out[y, x] = ((v >> 8) + v) >> 8
    return out


def apply_ops(frames, ops, masks):
    """vnf_overlay_draw in NumPy: frames (b,H,W,3) u8 (a copy is painted), ops a jpeg_encode.OP_DTYPE table in draw
    order, masks u8 -- every entry applied to its frame, one after the other"""
    out = np.asarray(frames, np.uint8).copy()
    b, h, w = out.shape[:3]
    for op in ops:
        f = int(op["frame"])
        if not 0 <= f < b:
            continue
        col = np.array([int(op["rgb"]) & 255, (int(op["rgb"]) >> 8) & 255, (int(op["rgb"]) >> 16) & 255], np.int64)
        x0, y0, x1, y1 = (int(op[k]) for k in ("x0", "y0", "x1", "y1"))
        yy, xx = np.mgrid[0:h, 0:w]
        if int(op["kind"]) == 0:
            inside = (xx >= x0) & (xx <= x1) & (yy >= y0) & (yy <= y1)
            hole = (xx >= x0 + 2) & (xx <= x1 - 2) & (yy >= y0 + 2) & (yy <= y1 - 2)
            out[f][inside & ~hole] = col
        elif int(op["kind"]) == 1:
            at = int(op["mask_offset"])
            if at < 0 or x1 <= 0 or y1 <= 0 or at + x1 * y1 > masks.size:
                continue
            m = masks[at:at + x1 * y1].reshape(y1, x1).astype(np.int64)
            cover = (xx >= x0) & (xx < x0 + x1) & (yy >= y0) & (yy < y0 + y1)
            ys, xs = np.nonzero(cover)
            a = m[ys - y0, xs - x0][:, None]
            v = out[f][ys, xs].astype(np.int64) * (255 - a) + col[None, :] * a + 128
            out[f][ys, xs] = ((v >> 8) + v) >> 8
    return out


# the frame and the faces of the overlay tests: name -> (boxes, names) on a (60,90,3) noise frame
def overlay_frame():
    return np.random.default_rng(7).integers(0, 256, (60, 90, 3), dtype=np.uint8)


OVERLAY_CASES = {
    "inside": ([(20.3, 15.7, 50.9, 45.2)], ["celeb_12"]),
    "negative_corners": ([(-5.6, -3.4, 30.2, 25.5)], ["celeb_3"]),
    "negative_corners_half": ([(-7.5, -8.5, 20.0, 20.0)], ["Unknown"]),
    "negative_anchor_x": ([(-30.5, 5.4, -2.3, 30.0)], ["celeb_77"]),
    "negative_anchor_y": ([(10.0, -3.6, 40.0, 20.0)], ["celeb_8"]),
    "label_off_right": ([(40.0, 10.0, 85.5, 40.0)], ["celeb_100"]),
    "label_off_bottom": ([(10.2, 55.3, 40.7, 58.9)], ["celeb_5"]),
    "box_off_bottom": ([(10.2, 30.0, 40.7, 80.0)], ["x"]),
    "two_overlapping": ([(10.0, 10.0, 50.0, 50.0), (30.5, 5.5, 70.5, 45.5)], ["celeb_1", "celeb_2"]),
    "wholly_outside": ([(100.0, 70.0, 130.0, 95.0), (-50.0, -50.0, -20.0, -20.0)], ["a", "b"]),
    "box_3px": ([(10.0, 10.0, 13.0, 13.0)], ["q"]),
    "box_4px": ([(30.9, 30.9, 34.2, 34.2)], ["q"]),
}
