"""The specification of vnf_overlay_draw_text in NumPy, written from Pillow's behaviour and not from the package's code.

What consecutive ImageDraw.text((x, y), s, fill=colour) calls with integer (x, y) and the default font paint on an RGB
frame, when that font is a FreeType face laid out by Layout.BASIC with integer advances and no kerning (Pillow 12.2.0:
size 10):

  * a glyph is what ImageDraw.text paints for the character alone: a coverage cut to its ink, the offset (ox, oy) of the
    cut from the anchor, and the advance font.getlength gives;
  * the coverage of a string is its glyphs composited left to right at pen positions equal to the sum of the preceding
    advances, combined as dst += round(src (255 - dst) / 255) where they overlap ('ff', 'fi', 'ft': plain add and max
    both differ from Pillow there);
  * the coverage m is pasted per channel as Pillow's paste does: v = bg (255 - m) + c m + 128, out = ((v >> 8) + v) >> 8;
  * everything is clipped to the frame; a later run paints over an earlier one.
"""
import numpy as np

FIRST, LAST = 32, 126            # printable ASCII
GREEN = (0, 255, 0)

_glyphs = None


def default_font():
    from PIL import Image, ImageDraw
    return ImageDraw.Draw(Image.new("L", (1, 1))).getfont()


def font_is_additive(font=None):
    """the premises above, as far as they can be read off the font object"""
    from PIL import ImageFont
    font = font if font is not None else default_font()
    if getattr(font, "layout_engine", None) != ImageFont.Layout.BASIC:
        return False
    return all(float(font.getlength(chr(c))).is_integer() for c in range(FIRST, LAST + 1))


def glyphs():
    """{character: (coverage (h,w) u8 cut to the ink, ox, oy, advance)} for printable ASCII"""
    global _glyphs
    if _glyphs is None:
        from PIL import Image, ImageDraw
        font = default_font()
        out, pad = {}, 40
        for c in range(FIRST, LAST + 1):
            im = Image.new("L", (3 * pad, 3 * pad), 0)
            ImageDraw.Draw(im).text((pad, pad), chr(c), fill=255, font=font)
            a = np.asarray(im)
            ys, xs = np.nonzero(a)
            adv = int(font.getlength(chr(c)))
            if ys.size == 0:
                out[chr(c)] = (np.zeros((0, 0), np.uint8), 0, 0, adv)
            else:
                y0, y1, x0, x1 = ys.min(), ys.max() + 1, xs.min(), xs.max() + 1
                out[chr(c)] = (a[y0:y1, x0:x1].copy(), int(x0) - pad, int(y0) - pad, adv)
        _glyphs = out
    return _glyphs


def round_div255(x):
    """round(x / 255) for integers x >= 0 (halves cannot occur: 255 is odd)"""
    return (2 * x + 255) // 510


def run_coverage(s):
    """-> (coverage (h,w) int64, ox, oy): the string's coverage and where its top-left pixel lies from the anchor;
    (None, 0, 0) for no ink"""
    g = glyphs()
    placed, pen = [], 0
    for ch in s:
        m, ox, oy, adv = g[ch]
        if m.size:
            placed.append((m.astype(np.int64), pen + ox, oy))
        pen += adv
    if not placed:
        return None, 0, 0
    x0, y0 = min(p[1] for p in placed), min(p[2] for p in placed)
    x1, y1 = max(p[1] + p[0].shape[1] for p in placed), max(p[2] + p[0].shape[0] for p in placed)
    cov = np.zeros((y1 - y0, x1 - x0), np.int64)
    for m, gx, gy in placed:
        dst = cov[gy - y0:gy - y0 + m.shape[0], gx - x0:gx - x0 + m.shape[1]]
        dst += round_div255(m * (255 - dst))
    return cov, x0, y0


def paste(frame, cov, px, py, colour=GREEN):
    """blend `colour` through the coverage whose top-left pixel goes to (px, py), in place, clipped to the frame"""
    h, w = frame.shape[:2]
    col = np.array(colour, np.int64)
    x0, y0, x1, y1 = max(px, 0), max(py, 0), min(px + cov.shape[1], w), min(py + cov.shape[0], h)
    if x1 <= x0 or y1 <= y0:
        return
    m = cov[y0 - py:y1 - py, x0 - px:x1 - px][:, :, None]
    bg = frame[y0:y1, x0:x1].astype(np.int64)
    v = bg * (255 - m) + col * m + 128
    frame[y0:y1, x0:x1] = np.where(m > 0, ((v >> 8) + v) >> 8, bg).astype(np.uint8)


def draw_text(frame, x, y, s, colour=GREEN):
    """ImageDraw.Draw(frame).text((x, y), s, fill=colour), in place"""
    cov, ox, oy = run_coverage(s)
    if cov is not None:
        paste(frame, cov, x + ox, y + oy, colour)


def draw_runs(frames, runs, colour=GREEN):
    """runs: (frame, x, y, string) in draw order on a copy of frames (b,H,W,3); a run that names a frame outside the
    batch is ignored"""
    out = np.asarray(frames, np.uint8).copy()
    for f, x, y, s in runs:
        if 0 <= f < out.shape[0]:
            draw_text(out[f], int(x), int(y), s, colour)
    return out


def emotion_lines(boxes, tags, probs, frame=0):
    """the text calls of cli_utils.draw_emotions (demo_image.py:161-171) for one frame: (frame, x, y, string)"""
    out = []
    for idx, box in enumerate(boxes):
        for i, (tag, p) in enumerate(zip(tags[idx], probs[idx])):
            out.append((frame, int(box[0] + 5), int(box[1]) + i * 16 + 4, '{} - {:.2f}%'.format(tag, p * 100)))
    return out


def draw_emotions(frame, boxes, tags, probs):
    return draw_runs(np.asarray(frame)[None], emotion_lines(boxes, tags, probs))[0]
