"""NumPy restatement of the device Huffman coder (csrc/jpeg_huff_device.h / .hip): what its passes must compute, stated
without them, so that the decomposition is pinned on a machine without a GPU.  The expected bytes are those of
vnf_jpeg_entropy_encode, the host coder, itself pinned to Pillow.

  sizes    every coding unit (one 8x8 block in scan order) -> its code as (value, nbits), from its own coefficients and
           the DC of the previous unit of its component, whose index is arithmetic in the unit's own
  scan     exclusive prefix sum of nbits -> bit offsets
  pack     OR every code into the zeroed stream at its offset, in any order; the last byte padded with 1-bits
  count    FF bytes of the stream
  scan     exclusive prefix sum -> ff_before(i)
  emit     header, stream byte i at header_len + i + ff_before(i) (a 00 follows every FF), FF D9

The Huffman tables are read from the DHT segments of the header the library writes, not typed in again.  This module
also holds the coefficient families and geometries the CPU and the GPU tests share.
"""
import numpy as np

from jpeg_encode_restatement import S420, S422, S444, geometry

OK, INVALID, CAPACITY = 0, -1, -4
HEADER_LEN = 623
MAX_UNIT_BITS = 20 + 63 * 26
FAMILIES = ("zero", "dense", "sparse_big", "tail63", "dcswing")
SIZES = [(1, 1), (8, 8), (17, 9), (8, 24), (33, 47), (64, 48), (130, 70), (264, 136)]       # (W, H)
SAMPLINGS = [S444, S422, S420]

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60,
                   61, 54, 47, 55, 62, 63])


def family(name, coef_count, seed=0):
    """one frame's coefficients, (coef_count,) int16; every family is inside the baseline range"""
    rng = np.random.default_rng(1000 * FAMILIES.index(name) + seed)
    c = np.zeros((coef_count // 64, 64), np.int16)
    if name == "dense":
        c[:] = rng.integers(-1023, 1024, c.shape)
    elif name == "sparse_big":
        c[:] = np.where(rng.random(c.shape) < 0.06, rng.integers(-1023, 1024, c.shape), 0)
    elif name == "tail63":
        c[:, 63] = rng.integers(1, 1024, c.shape[0])
        c[:, 0] = rng.integers(-1000, 1000, c.shape[0])
    elif name == "dcswing":
        c[:, 0] = np.where(np.arange(c.shape[0]) & 1, 1023, -1024)
    else:
        assert name == "zero"
    return c.reshape(-1)


def enough_capacity(units):
    """a capacity every frame of `units` coding units fits: header, the longest scan with every byte stuffed, EOI"""
    return HEADER_LEN + 2 * -(-MAX_UNIT_BITS * units // 8) + 4


def huffman_tables(header):
    """{(class, id): {symbol: (code, length)}} from the DHT segments of a JPEG header (T.81 annex C)"""
    header = bytes(header)
    out, at = {}, 2
    while at < len(header):
        assert header[at] == 0xFF
        marker, n = header[at + 1], int.from_bytes(header[at + 2:at + 4], "big")
        if marker == 0xC4:
            tc, th = header[at + 4] >> 4, header[at + 4] & 15
            counts, syms = header[at + 5:at + 21], header[at + 21:at + 2 + n]
            table, code, k = {}, 0, 0
            for length in range(1, 17):
                for _ in range(counts[length - 1]):
                    table[syms[k]] = (code, length)
                    code, k = code + 1, k + 1
                code <<= 1
            out[(tc, th)] = table
        at += 2 + n
    return out


class Invalid(Exception):
    pass


def _category(v):
    return int(abs(int(v))).bit_length()


def _low_bits(v, cat):
    return (v - 1 if v < 0 else v) & ((1 << cat) - 1)


def unit_code(blk, pred, dc, ac):
    """T.81 F.1.2 for one block (natural order) -> (value, nbits) as Python ints"""
    value = nbits = 0

    def put(v, k):
        nonlocal value, nbits
        value, nbits = (value << k) | v, nbits + k

    diff = int(blk[0]) - pred
    cat = _category(diff)
    if cat > 11:
        raise Invalid
    code, length = dc[cat]
    put((code << cat) | _low_bits(diff, cat), length + cat)
    z = blk[ZIGZAG]
    last = 0
    for k in np.flatnonzero(z[1:]) + 1:
        k, v = int(k), int(z[k])
        run = k - last - 1
        while run > 15:                                  # ZRL
            put(*ac[0xF0])
            run -= 16
        cat = _category(v)
        if cat > 10:
            raise Invalid
        code, length = ac[(run << 4) | cat]
        put((code << cat) | _low_bits(v, cat), length + cat)
        last = k
    if last != 63:                                       # EOB
        put(*ac[0x00])
    return value, nbits


def scan_units(w, h, sampling):
    """per coding unit in scan order: (component, first coefficient, index of the previous unit of the component or
    -1), the last by arithmetic on the unit's own index, as the kernels find it"""
    hf, vf, bw, bh, _ = geometry(w, h, sampling)
    plane = [0, 64 * bw[0] * bh[0], 64 * (bw[0] * bh[0] + bw[1] * bh[1])]
    mx, luma = bw[1], hf * vf
    upm = luma + 2
    units = []
    for u in range(bw[1] * bh[1] * upm):
        m, r = divmod(u, upm)
        y, x = divmod(m, mx)
        if r < luma:
            by, bx = divmod(r, hf)
            c, at = 0, plane[0] + ((y * vf + by) * bw[0] + x * hf + bx) * 64
            pred = u - 1 if r > 0 else (m - 1) * upm + luma - 1 if m > 0 else -1
        else:
            c = 1 + r - luma
            at = plane[c] + (y * bw[c] + x) * 64
            pred = u - upm if m > 0 else -1
        units.append((c, at, pred))
    return units


def encode(coefs, w, h, sampling, header, capacity=None, seed=0):
    """the passes above -> (status, length, the file's first min(length, capacity) bytes)"""
    tables = huffman_tables(header)
    units = scan_units(w, h, sampling)
    # sizes
    codes = []
    try:
        for c, at, pred in units:
            t = 1 if c else 0
            codes.append(unit_code(coefs[at:at + 64], int(coefs[units[pred][1]]) if pred >= 0 else 0, tables[(0, t)], tables[(1, t)]))
    except Invalid:
        return INVALID, None, None
    bits = np.array([n for _, n in codes], np.int64)
    assert bits.max() <= MAX_UNIT_BITS
    # scan
    offsets = np.concatenate([[0], np.cumsum(bits)[:-1]])
    total = int(bits.sum())
    padded = -(-total // 8) * 8
    # pack: OR in a shuffled order; the padding of the last byte by whoever comes to it
    stream = (1 << (padded - total)) - 1
    for u in np.random.default_rng(seed).permutation(len(units)):
        stream |= codes[u][0] << (padded - int(offsets[u]) - int(bits[u]))
    data = np.frombuffer(stream.to_bytes(padded // 8, "big"), np.uint8)
    # count, scan
    ff = data == 0xFF
    before = np.cumsum(ff) - ff
    # emit
    length = len(header) + data.size + int(ff.sum()) + 2
    out = np.zeros((length,), np.uint8)
    out[:len(header)] = np.frombuffer(bytes(header), np.uint8)
    out[len(header) + np.arange(data.size) + before] = data
    out[-2:] = (0xFF, 0xD9)
    if capacity is None or length <= capacity:
        return OK, length, out.tobytes()
    return CAPACITY, length, out[:capacity].tobytes()
