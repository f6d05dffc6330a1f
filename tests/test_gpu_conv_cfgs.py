"""Every tile configuration behind launch_conv, in every storage layout it is compiled for, one launch at a time through
the one-convolution probe (vnf_conv_probe_*), against the float64 restatement of tests/conv_reference.py.

Two data classes per (shape, dtype), every admitted configuration id in both, plus the VNF_WS_PERSIST=0 twin of every
admitted wave-specialised id:
  exact    operands on dyadic grids (conv_reference.exact_data): the sum has ONE value whatever the tile, the K order or
           the MFMA shape, so every configuration must give the reference's bits over the whole segment -- no tolerance;
  generic  seeded normal operands: (a) all configurations and twins give the same bits; (b) those bits are within
           conv_reference.generic_bar of float64 on the stored values.
In both: every byte outside the written region (other columns, rows >= M, the input and residual buffers) keeps its
sentinel, and the same id twice gives the same bits.

Largest |got - want| / bar of the generic class on the MI355X (256 CUs), per dtype, over the table and case P -- the
bar is conv_reference.generic_bar, from the kernel guide's fp32-chain figure and the number formats, not from these:
  f32 0.517   f16x2 0.149   f16p 0.240   bf16 1.000   f16 0.998
(a 16-bit store within its half unit of an expected value that sits just outside the fp32 slack of a tie is at ratio
~1 by construction; the 4-byte layouts show the fp32 chain itself: half the bar at most.)  Launches of that run, per
dtype, table + case P: f32 3060, bf16 3080 + 174, f16 3080 + 174, f16x2 4302, f16p 4278 + 171; no id excluded; no
configuration found wrong.

A launch that returns an error ends this process's GPU work at once (pytest.exit): the last line of the progress file
names what was running."""
import contextlib
import ctypes
import os

import pytest
import torch

import conv_reference as cr
from conv_reference import CASES, DTYPES, SPLIT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -1            # all ones: a NaN in every layout, never a value of the data
PAD_ROWS = 3             # rows behind M in every output and residual buffer
FAMILY = ("ring", "patch", "ws")
# ids that no small legal shape admits, per dtype, with the conv_cfg_ok clause that excludes them: none -- case B
# (3x3, Cout = 192 in a 256-wide weight image) admits all 78 in all five layouts
EXCLUDED = {dt: {} for dt in DTYPES}
LAUNCHES = {dt: 0 for dt in DTYPES}


def _lib():
    from vn_celeb_face_recognition_amd import _lib as L
    return L


def _code(dt):
    L = _lib()
    return {"f32": (L.VNF_F32, 0), "bf16": (L.VNF_BF16, 0), "f16": (L.VNF_F16, 0), "f16x2": (L.VNF_F16X2, 0), "f16p": (L.VNF_F16X2, 1)}[dt]


def _tile(cfg):
    t = (ctypes.c_int32 * 6)()
    _lib().check(_lib().load().vnf_conv_cfg_tile(cfg, t))
    return dict(zip(("family", "bm", "bn", "wm", "wn", "stages"), t))


def _f32p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@contextlib.contextmanager
def _persist(on):
    """VNF_WS_PERSIST as a probe reads it when it is created."""
    old = os.environ.get("VNF_WS_PERSIST")
    if not on:
        os.environ["VNF_WS_PERSIST"] = "0"
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("VNF_WS_PERSIST", None)
        else:
            os.environ["VNF_WS_PERSIST"] = old


def _geom_struct(g, dt):
    L = _lib()
    code, planar = _code(dt)
    s = L.ConvProbeGeom(n=g.n, h=g.H, w=g.W, cin=g.Cin, kh=g.KH, kw=g.KW, sh=g.sh, sw=g.sw, ph=g.ph, pw=g.pw, cout=g.Cout,
                        x_coff=g.x_coff, ldx=g.ldx, nseg=len(g.segs), has_res=int(g.res is not None),
                        ldres=g.res[0] if g.res else 0, res_coff=g.res[1] if g.res else 0, act=g.act, out_f32=int(g.out_f32),
                        dtype=code, planar=planar)
    for i, (c0, c1, ld, coff) in enumerate(g.segs):
        s.seg_c0[i], s.seg_c1[i], s.seg_ld[i], s.seg_coff[i] = c0, c1, ld, coff
    return s


def _create(g, dt, d, persist=True):
    """(rc, handle) of vnf_conv_probe_create on the data set's host fp32 parameters."""
    host = [None if t is None else t.float().contiguous() for t in (d.w, d.bias, d.slope, d.pre_s, d.pre_t)]
    h = ctypes.c_void_p()
    with _persist(persist):
        rc = _lib().load().vnf_conv_probe_create(ctypes.byref(_geom_struct(g, dt)), *[_f32p(t) for t in host], ctypes.byref(h))
    return rc, h


class Probe:
    def __init__(self, g, dt, d, persist=True):
        L = _lib()
        rc, self.h = _create(g, dt, d, persist)
        L.check(rc)
        self.g, self.dt = g, dt
        adm = (ctypes.c_int32 * 256)()
        fam = (ctypes.c_int32 * 3)()
        self.total = L.load().vnf_conv_probe_cfgs(self.h, adm, 256, fam)
        assert self.total == sum(fam) > 0
        self.families = list(fam)
        self.admitted = [c for c in range(self.total) if adm[c]]

    def family(self, cfg):
        return 0 if cfg < self.families[0] else 1 if cfg < self.families[0] + self.families[1] else 2

    def run(self, cfg, x, outs, res):
        arr = (ctypes.c_void_p * 4)(*[o.data_ptr() for o in outs])
        return _lib().load().vnf_conv_probe_run(self.h, cfg, ctypes.c_void_p(x.data_ptr()), arr, _f32p(res), _lib().current_stream_ptr())

    def close(self):
        if self.h:
            _lib().load().vnf_destroy(self.h)
            self.h = None


class Buffers:
    """The device buffers of one (geometry, dtype, data set): inputs in the layout with the sentinel around the slices,
    and one output buffer per segment."""
    def __init__(self, g, dt, d, raw=None):   # raw: (x, res) already encoded
        od = cr.out_dtype(g, dt)
        x = torch.full((g.n, g.H, g.W, g.ldx), SENTINEL, dtype=cr.raw_dtype(dt))
        x[..., g.x_coff:g.x_coff + g.Cin] = raw[0] if raw else cr.encode(d.x, dt)
        self.x, self.x_keep = x.to(DEV), x.to(DEV)
        self.res = self.res_keep = None
        if g.res is not None:
            r = torch.full((g.M + PAD_ROWS, g.res[0]), SENTINEL, dtype=cr.raw_dtype(dt))
            r[:g.M, g.res[1]:g.res[1] + g.Cout] = raw[1] if raw else cr.encode(d.res, dt)
            self.res, self.res_keep = r.to(DEV), r.to(DEV)
        self.outs = [torch.empty((g.M + PAD_ROWS, ld), dtype=cr.raw_dtype(od), device=DEV) for _, _, ld, _ in g.segs]

    def clear(self):
        for o in self.outs:
            o.fill_(SENTINEL)

    def inputs_untouched(self):
        return torch.equal(self.x, self.x_keep) and (self.res is None or torch.equal(self.res, self.res_keep))


class Sweep:
    """Runs configurations of one probe pair (persistent switch on / off) over one Buffers and keeps the books."""
    def __init__(self, g, dt, d, progress, label, raw=None):
        self.g, self.dt, self.d, self.progress, self.label = g, dt, d, progress, label
        self.buf = Buffers(g, dt, d, raw)
        self.probe = Probe(g, dt, d, True)
        self.twin = Probe(g, dt, d, False)
        assert self.twin.admitted == self.probe.admitted
        self.launches = 0

    def close(self):
        self.probe.close()
        self.twin.close()

    def launch(self, cfg, twin=False):
        p = self.twin if twin else self.probe
        self.buf.clear()
        with open(self.progress, "a") as f:
            f.write("%s %s %s cfg %d%s\n" % (self.label, self.dt, self.d.note, cfg, " one-tile twin" if twin else ""))
            f.flush()
        rc = p.run(cfg, self.buf.x, self.buf.outs, self.buf.res)
        if rc != 0:
            msg = _lib().load().vnf_last_error().decode("utf-8", "replace")
            pytest.exit("conv probe launch failed (%d: %s) at the last line of %s: %s %s %s cfg %d; no further GPU work"
                        % (rc, msg, self.progress, self.label, self.dt, self.d.note, cfg), returncode=3)
        self.launches += 1
        LAUNCHES[self.dt] += 1
        return [o.clone() for o in self.buf.outs]

    def runs(self):
        """(cfg, twin) of every launch the sweep owes: each admitted id, the heuristic, each wave-specialised id's twin."""
        for cfg in [-1] + self.probe.admitted:
            yield cfg, False
            if cfg >= 0 and self.probe.family(cfg) == 2:
                yield cfg, True

    def describe(self, cfg, twin):
        if cfg < 0:
            return "heuristic"
        t = _tile(cfg)
        return "cfg %d (%s %dx%d, %dx%d waves, %d stages%s)" % (cfg, FAMILY[t["family"]], t["bm"], t["bn"], t["wm"], t["wn"], t["stages"],
                                                                ", VNF_WS_PERSIST=0" if twin else "")


def _first_difference(g, dt, got, want, what):
    """'(m, c) got / want' of the first differing element of the first differing buffer (raw bits and values)."""
    od = cr.out_dtype(g, dt)
    mask = 0xffff if cr.ELEM_BYTES[od] == 2 else 0xffffffff
    for i, (a, b) in enumerate(zip(got, want)):
        a, b = a.cpu(), b.cpu()
        if torch.equal(a, b):
            continue
        m, c = [int(v) for v in (a != b).nonzero()[0]]
        c0, c1, ld, coff = g.segs[i]
        where = "segment %d row m = %d buffer column %d" % (i, m, c)
        inside = m < g.M and coff <= c < coff + c1 - c0
        if inside:
            where += " = output channel %d" % (c0 + c - coff)
            if od == "f16p":   # a planar column is half of an 8-channel unit: show the unit's first channel
                u = coff + (c - coff) // 8 * 8
                ga, gb = cr.decode(a[m:m + 1, u:u + 8], od)[0], cr.decode(b[m:m + 1, u:u + 8], od)[0]
                return "%s: %s, unit got %s want %s" % (what, where, ga.tolist(), gb.tolist())
            return "%s: %s, got %r (bits %#x) want %r (bits %#x)" % (
                what, where, cr.decode(a[m:m + 1, c:c + 1], od).item(), int(a[m, c]) & mask, cr.decode(b[m:m + 1, c:c + 1], od).item(),
                int(b[m, c]) & mask)
        return "%s: %s is OUTSIDE the written region and lost its sentinel: bits %#x" % (what, where, int(a[m, c]) & mask)
    return None


def _check_exact(sw, v):
    g, dt = sw.g, sw.dt
    want = [b.to(DEV) for b in cr.expected_buffers(g, dt, v, g.M + PAD_ROWS, SENTINEL)]
    for cfg, twin in sw.runs():
        for rep in range(2):
            got = sw.launch(cfg, twin)
            if not all(torch.equal(a, b) for a, b in zip(got, want)):
                pytest.fail(_first_difference(g, dt, got, want, "%s %s exact[%s] %s, run %d" % (sw.label, dt, sw.d.note, sw.describe(cfg, twin), rep)))
            assert sw.buf.inputs_untouched(), "%s %s %s wrote to its input or residual" % (sw.label, dt, sw.describe(cfg, twin))


def _check_generic(sw, v, absum):
    g, dt = sw.g, sw.dt
    od = cr.out_dtype(g, dt)
    base = base_name = None
    for cfg, twin in sw.runs():
        for rep in range(2):
            got = sw.launch(cfg, twin)
            assert sw.buf.inputs_untouched(), "%s %s %s wrote to its input or residual" % (sw.label, dt, sw.describe(cfg, twin))
            if base is None:
                base, base_name = got, sw.describe(cfg, twin)
                # outside the segments the sentinel, inside none of it
                shape = [torch.full((g.M + PAD_ROWS, ld), SENTINEL, dtype=cr.raw_dtype(od)) for _, _, ld, _ in g.segs]
                for b, s, (c0, c1, ld, coff) in zip(base, shape, g.segs):
                    b = b.cpu()
                    s[:g.M, coff:coff + c1 - c0] = b[:g.M, coff:coff + c1 - c0]
                    assert torch.equal(b, s), _first_difference(g, dt, [b], [s], "%s %s generic %s" % (sw.label, dt, base_name))
                continue
            if not all(torch.equal(a, b) for a, b in zip(got, base)):
                pytest.fail(_first_difference(g, dt, got, base, "%s %s generic %s, run %d, against %s" % (sw.label, dt, sw.describe(cfg, twin), rep, base_name)))
    out = torch.cat([cr.decode(b.cpu()[:g.M, coff:coff + c1 - c0].contiguous(), od) for b, (c0, c1, ld, coff) in zip(base, g.segs)], dim=1)
    assert torch.isfinite(out).all()
    ratio = (out - v).abs() / cr.generic_bar(g, dt, v, absum)
    worst = ratio.max().item()
    if worst > 1:
        m, c = [int(t) for t in (ratio == ratio.max()).nonzero()[0]]
        pytest.fail("%s %s generic: |got - want| is %.3f of the bar at (m, c) = (%d, %d): got %r want %r" % (sw.label, dt, worst, m, c, out[m, c].item(), v[m, c].item()))
    return worst


def _data_sets(g, dt, only=None):
    sets = []
    if not (dt in SPLIT and g.K > cr.EXACT_MAX_K_SPLIT):
        for which in cr.exact_sets(dt):
            if only not in (None, which):
                continue
            d = cr.exact_data(g, dt, which)
            rounded = cr.exact_self_check(g, dt, d)     # rejects a set that is not exact
            assert rounded > 0 or not cr.rounding_can_bite(g, dt), "no expected output needs rounding"
            sets.append(d)
    if only in (None, "generic"):
        sets.append(cr.generic_data(g, dt))
    return sets


PAIRS = [(case, dt) for case in CASES for dt in DTYPES if any(cr.with_dtype_alignment(g, dt) for g in CASES[case])]


@pytest.mark.parametrize("case,dt", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_every_admitted_configuration(case, dt, tmp_path):
    progress = str(tmp_path / "progress.txt")
    worst, launches, ids = 0.0, 0, set()
    for g in CASES[case]:
        if cr.with_dtype_alignment(g, dt) is None:
            continue
        for d in _data_sets(g, dt):
            v, absum = cr.conv_pre_store(g, dt, d)
            sw = Sweep(g, dt, d, progress, g.name)
            try:
                assert sw.probe.admitted, "no configuration admitted"
                ids.update(sw.probe.admitted)
                if d.note == "generic":
                    worst = max(worst, _check_generic(sw, v, absum))
                else:
                    _check_exact(sw, v)
                # an id conv_cfg_ok rejects is refused, never replaced by the heuristic
                refused = [c for c in range(sw.probe.total) if c not in sw.probe.admitted]
                for c in refused[:2] + [sw.probe.total, -2]:
                    assert sw.probe.run(c, sw.buf.x, sw.buf.outs, sw.buf.res) == -1
                launches += sw.launches
            finally:
                sw.close()
    print("conv cfgs %s %s: %d launches over %d ids, generic worst ratio to the bar %.3f" % (case, dt, launches, len(ids), worst))


def test_pre_bn_geometries_the_bias_table_is_wrong_for_are_refused():
    L = _lib()
    for g in cr.REFUSED:
        for dt in ("f32", "bf16", "f16p"):
            rc, h = _create(g, dt, cr.generic_data(g, dt))
            assert rc == -1 and not h.value, (g.name, dt, rc)
            assert b"pre-conv BatchNorm" in L.load().vnf_last_error()
            # the same geometry without the BatchNorm is a legal convolution
            g2 = cr.replace(g, pre_bn=False)
            rc, h = _create(g2, dt, cr.generic_data(g2, dt))
            assert rc == 0
            L.load().vnf_destroy(h)


def test_every_configuration_is_admitted_somewhere():
    """Per dtype, the union over the shape table of the admitted ids is the whole range but for EXCLUDED: the sweep above
    runs every admitted id, so it reaches every instantiation.  Ring ids 17 and 28 are the same tuple; both are ids."""
    for dt in DTYPES:
        union, total = set(), None
        for case in CASES.values():
            for g in case:
                if cr.with_dtype_alignment(g, dt) is None:
                    continue
                p = Probe(g, dt, cr.generic_data(g, dt))
                union.update(p.admitted)
                total = p.total
                p.close()
        assert _tile(17) == _tile(28)
        missing = set(range(total)) - union
        assert missing == set(EXCLUDED[dt]), (dt, sorted(missing))
        print("conv cfgs %s: %d of %d ids admitted by the table, excluded %s; launches so far in this process %d"
              % (dt, len(union), total, sorted(EXCLUDED[dt]) or "none", LAUNCHES[dt]))


# ------------------------------------------------------------------------------------------------ case P
def _ws_ids():
    ids, c = [], 0
    t = (ctypes.c_int32 * 6)()
    while _lib().load().vnf_conv_cfg_tile(c, t) == 0:
        if t[0] == 2:
            ids.append(c)
        c += 1
    return ids


def _persistent_compiled(dt, t):   # launch_one in csrc/conv_ws.hip
    return dt in ("bf16", "f16", "f16p") and (t["bn"] // t["wn"] // 16) % 2 == 0


def _res_form(dt, t):              # the RES = true instantiation: 2-byte types, small tiles
    return dt in ("bf16", "f16") and (t["bm"] // t["wm"] // 16) * (t["bn"] // t["wn"] // 32) <= 8


def _walk_shape(dt, t, cus):
    """(Cout, M, nblk, slots) of the smallest 1x1 over Cin = 64 whose tiles outnumber the persistent grid."""
    nkt = -(-64 // (128 // cr.ELEM_BYTES[dt]))
    lds = t["stages"] * (t["bm"] + t["bn"]) * 128 + nkt * 8 * 16
    slots = cus * (2 if lds <= 80 * 1024 else 1)
    for cout in (896, 768):   # 896 where its weight image (7 x 128 rows) holds whole tiles of the id's BN, else 768 (BN = 192, 256)
        tiles_n = -(-cout // t["bn"])
        if tiles_n * t["bn"] <= -(-cout // 128) * 128:
            break
    tiles_m = slots // tiles_n + 1
    M = (tiles_m - 1) * t["bm"] + t["bm"] // 2 + 1
    return cout, M, tiles_m * tiles_n, slots


WALKS = [(dt, which) for dt in ("bf16", "f16", "f16p") for which in cr.exact_sets(dt) + ("generic",)]


@pytest.mark.parametrize("dt,which", WALKS, ids=["%s-%s" % w for w in WALKS])
def test_persistent_workgroups_walk_from_tile_to_tile(dt, which, tmp_path):
    """Every wave-specialised id whose persistent form is compiled for the dtype, with more tiles than its grid
    (nblk > CUs * (lds <= 80 KiB ? 2 : 1)) so that workgroups really take a second tile: a 1x1 over Cin = 64 with M just
    over grid * BM / ceil(Cout / BN) and not a multiple of BM, without a residual and -- where the RES form exists --
    with one.  The rows of a 1x1 are independent, so one data set of the largest M serves every id: exact data against
    the reference's bits; generic data against the bits the ids before it gave for the same rows (twins included), and
    the rows together against the bar.  Each id runs twice, then its one-tile twin; one data set per test case."""
    progress = str(tmp_path / "progress.txt")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ids = _ws_ids()
    tiles = {c: _tile(c) for c in ids}
    assert all(_persistent_compiled(dt, t) for t in tiles.values())
    shapes = {c: _walk_shape(dt, tiles[c], cus) for c in ids}
    worst, launches, walked = 0.0, 0, {False: set(), True: set()}
    for with_res in (False, True):
        todo = [c for c in ids if not with_res or _res_form(dt, tiles[c])]
        if not todo:
            continue
        full = cr.persistent_geom(max(shapes[c][1] for c in todo), 896, with_res)
        for d_full in _data_sets(full, dt, only=which):
            v_full, absum_full = cr.conv_pre_store(full, dt, d_full)
            x_raw = cr.encode(d_full.x, dt)
            want, base, res_raw = {}, {}, {}
            for c in todo:
                cout, M, nblk, slots = shapes[c]
                assert nblk > slots and M % tiles[c]["bm"]
                if cout not in want:
                    want[cout] = cr.encode(v_full[:, :cout].contiguous(), dt).to(DEV)
                    base[cout] = [torch.empty_like(want[cout]), 0]       # generic: the rows seen so far, and how many
                    res_raw[cout] = None if d_full.res is None else cr.encode(d_full.res[:, :cout].contiguous(), dt)
                g = cr.persistent_geom(M, cout, with_res)
                d = cr.Data(x=d_full.x[:, :, :M], w=d_full.w[:cout], bias=d_full.bias[:cout], q=d_full.q, note=d_full.note,
                            res=None if d_full.res is None else d_full.res[:M, :cout])
                sw = Sweep(g, dt, d, progress, g.name, raw=(x_raw[:, :, :M], None if d_full.res is None else res_raw[cout][:M]))
                try:
                    assert c in sw.probe.admitted, (c, g.name)
                    pad = torch.full((PAD_ROWS, cout), SENTINEL, dtype=cr.raw_dtype(dt), device=DEV)
                    for rep, twin in enumerate((False, False, True)):
                        got = sw.launch(c, twin)[0]
                        rows, known = base[cout]
                        if d.note == "generic":
                            rows[known:M] = got[known:M]
                            base[cout][1] = known = max(known, M)
                            ref, what = rows, "generic, against the ids before it"
                        else:
                            ref, what = want[cout], "exact[%s]" % d.note
                        expect = torch.cat([ref[:M], pad])
                        if not torch.equal(got, expect):
                            pytest.fail(_first_difference(g, dt, [got], [expect], "%s %s %s %s, run %d" % (g.name, dt, what, sw.describe(c, twin), rep)))
                        assert sw.buf.inputs_untouched()
                    launches += sw.launches
                    walked[with_res].add(c)
                finally:
                    sw.close()
            for cout, (rows, known) in base.items():
                if d_full.note == "generic" and known:
                    out = cr.decode(rows[:known].cpu(), dt)
                    ratio = (out - v_full[:known, :cout]).abs() / cr.generic_bar(full, dt, v_full[:known, :cout], absum_full[:known, :cout])
                    assert torch.isfinite(out).all() and ratio.max().item() <= 1, (cout, ratio.max().item())
                    worst = max(worst, ratio.max().item())
    assert walked[False] == set(ids)
    assert walked[True] == {c for c in ids if _res_form(dt, tiles[c])} and (walked[True] or dt == "f16p")
    print("conv cfgs P %s %s: %d launches, %d ids without and %d with a residual, %d CUs, generic worst ratio to the bar %.3f"
          % (dt, which, launches, len(walked[False]), len(walked[True]), cus, worst))
