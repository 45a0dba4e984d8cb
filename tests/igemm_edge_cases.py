"""Geometries at the edges of plan_conv (csrc/igemm.hip: k_igemm, k_igemm_halo, k_igemm_small, k_igemm_wide, k_igemm_queue,
k_dense64), shared by tests/test_igemm_edge_cases.py (CPU: every case engages the plan it is listed for and keeps the corner
it was written for) and tests/test_gpu_igemm_edges.py (the kernels against fp64) -- TEST ONLY.

A case is a dict: name, mode, ind / outd / k / s / p (3-tuples d, h, w), cin, cout, in_stride / out_stride (None: dense),
ps / ps_channels (pixel-shuffle store), in_bn (None, True, or the (lo, hi) range its shifts are drawn from), in_relu, bias,
out_relu, accumulate, gate, stats (None, "table", "sink": a forward sink with moving statistics, "bwd table", "bwd sink") with
bwd_relu, fold (None, "relu", "linear": lisec_conv_extras.in_y with / without in_fold_relu), tail, dense_dw,
rows = (capacity, device count) and queue, flags (names of ops flags such as "SMALL_TILE"), splitk, knobs (lisec_tuning fields
to set for the call), like (the name of the case whose operands it shares: twins that differ in the launch form only), plan
(the fields of ops.conv_plan the case MUST give; queried on the host, 256 CUs) and facts (the geometric reasons the case is in
the table; facts_of(case) restates them FROM THE DIMS, not from the planner).
Inputs are default_rng(crc32(name)) normals, float32; kernels are scaled by 1 / sqrt(taps * cin)."""
import zlib

import numpy as np

from wgrad_edge_cases import bn_state, tuning          # noqa: F401  (tuning: re-exported for the two test files)
from wino_edge_cases import source_plane

K133, K113, K333, K111, K313, K144, K122 = (1, 3, 3), (1, 1, 3), (3, 3, 3), (1, 1, 1), (3, 1, 3), (1, 4, 4), (1, 2, 2)
S1, S122, S211, S222, S144 = (1, 1, 1), (1, 2, 2), (2, 1, 1), (2, 2, 2), (1, 4, 4)
P011, P001, P111, P101, P0 = (0, 1, 1), (0, 0, 1), (1, 1, 1), (1, 0, 1), (0, 0, 0)
POS = (0.5, 1.5)              # shifts in (0.5, 1.5): a padding or halo position that wrongly received the affine is positive
BM = 128

_DEFAULTS = dict(in_stride=None, out_stride=None, ps=0, ps_channels=0, in_bn=None, in_relu=False, bias=None, out_relu=False,
                 accumulate=False, gate=False, stats=None, bwd_relu=False, fold=None, tail=False, dense_dw=False, rows=None,
                 queue=False, flags=(), splitk=True, knobs=None, facts=None, like=None)


def _case(name, mode, ind, outd, k, s, p, cin, cout, plan, **kw):
    assert set(kw) <= set(_DEFAULTS), set(kw) - set(_DEFAULTS)
    c = dict(_DEFAULTS, name=name, mode=mode, ind=ind, outd=outd, k=k, s=s, p=p, cin=cin, cout=cout, plan=plan, **kw)
    if c["bias"] is None:
        c["bias"] = mode == 0 and not c["fold"]
    c["knobs"], c["facts"] = dict(c["knobs"] or {}), dict(c["facts"] or {})
    return c


def _same(name, mode, dims, k, p, cin, cout, plan, **kw):
    """a stride-1 case whose output map is its input map"""
    return _case(name, mode, dims, dims, k, S1, p, cin, cout, plan, **kw)


def _plan(kernel, **kw):
    return dict(kernel=kernel, **kw)


NO_DB_2, NO_DB_3 = dict(lone_db=0, force_splitk=2), dict(lone_db=0, force_splitk=3)
IGEMM1 = _plan("igemm", k_slices=1, cols=64, launches=1)

# ---- the geometries whose plans were read at the parent commit ------------------------------------------------------------------
CASES = [
    _case("plain one row", 0, (1, 1, 1), (1, 1, 1), K133, (1, 1, 1), P011, 4, 1, dict(IGEMM1, workgroups=1, tiles=1),
          facts=dict(last_tile_rows=1, last_block_cols=1, partial_slab=4)),
    # M = 129: the second tile holds one row; 68 channels = one slab + 4, 65 columns = one block + 1
    _same("plain M129", 0, (1, 3, 43), K133, P011, 68, 65, dict(IGEMM1, tiles=2, workgroups=4), in_stride=72, out_stride=72,
          in_bn=True, in_relu=True, facts=dict(last_tile_rows=1, last_block_cols=1, partial_slab=4, max_lines=3)),
    # 60 rows over three depths in one tile: tap_live must not skip a depth tap because the FIRST row's plane lacks it
    _case("plain 3D", 0, (5, 7, 9), (3, 4, 5), K333, S222, P111, 64, 64,
          _plan("igemm", k_slices=9, double_buffered=1, tiles=1), facts=dict(crosses_depth=True, depth_taps=[2, 3, 2])),
    _case("k4 s4 transposed", 1, (1, 3, 5), (1, 12, 20), K144, S144, P0, 64, 64,
          _plan("igemm", k_slices=5, double_buffered=1, parity_classes=0, tiles=2), facts=dict(last_tile_rows=112)),
    _case("stride-2 gradient odd map", 1, (1, 5, 7), (1, 9, 13), K133, S122, P011, 64, 64,
          _plan("igemm", parity_classes=0, tiles=1), facts=dict(last_tile_rows=117)),
    _same("lone slices", 0, (1, 13, 25), K133, P011, 96, 128,
          _plan("igemm", k_slices=3, double_buffered=0, workgroups=18, cols=64), knobs=NO_DB_3,
          facts=dict(last_tile_rows=69, partial_slab=32)),
    _same("half-N 128", 0, (1, 13, 25), K133, P011, 96, 128, _plan("igemm", cols=32, k_slices=1, workgroups=12), knobs=NO_DB_2,
          facts=dict(last_tile_rows=69, last_block_cols=64)),
    # 40 columns: the second half of the only 64-column block holds 8, and no workgroup exists for a third or fourth half
    _same("half-N 40", 0, (1, 13, 25), K133, P011, 96, 40, _plan("igemm", cols=32, k_slices=1, workgroups=6), knobs=NO_DB_2,
          facts=dict(last_block_cols=40, last_half_cols=8)),
    _same("half-N 16", 0, (1, 13, 25), K133, P011, 96, 16, _plan("igemm", cols=32, k_slices=1, workgroups=3), knobs=NO_DB_2,
          facts=dict(last_block_cols=16, last_half_cols=16)),
]

# the w-halo widths: 64, 65 and 125 run the three-line kernel, 126 .. 129 the two-line one; sliced (3 slices on two images) and
# in one pass.  (Three lines high, none of these maps puts three lines into one tile: the cases behind the loop do.)
for _w, _kernel, _tiles, _lines in [(64, "halo3", 2, 2), (65, "halo3", 2, 2), (125, "halo3", 3, 2), (126, "halo2", 3, 2),
                                    (127, "halo2", 3, 2), (128, "halo2", 3, 1), (129, "halo2", 4, 2)]:
    _f = dict(max_lines=_lines, last_tile_rows=3 * _w - (_tiles - 1) * BM)
    CASES.append(_same(f"halo W{_w} sliced", 0, (1, 3, _w), K133, P011, 64, 64,
                       _plan(_kernel, k_slices=3, double_buffered=1, tiles=_tiles, cols=64), in_bn=POS, in_relu=True, facts=_f))
    CASES.append(_same(f"halo W{_w}", 0, (1, 3, _w), K133, P011, 64, 64,
                       _plan(_kernel, k_slices=1, double_buffered=0, tiles=_tiles, cols=64), in_bn=POS, in_relu=True,
                       splitk=False, facts=_f))

CASES += [
    # the narrowest and the widest map whose tiles touch three lines: tile 1 of W 65 holds 2 + 65 + 61 rows; tile 41 of W 125 starts
    # at w = 123: a = 2 rows on its first line, 125 on the second, 1 on the third
    _same("halo3 W65 three lines", 0, (1, 5, 65), K133, P011, 64, 64, _plan("halo3", k_slices=1, tiles=3), in_bn=POS, in_relu=True,
          splitk=False, facts=dict(max_lines=3, last_tile_rows=69)),
    _same("halo3 W125 three lines", 0, (1, 44, 125), K133, P011, 64, 64, _plan("halo3", k_slices=1, tiles=43), in_bn=POS,
          in_relu=True, splitk=False, facts=dict(max_lines=3, last_tile_rows=124)),
    _case("halo3 3D strided", 0, (3, 2, 70), (2, 2, 70), K333, S211, P111, 80, 72, _plan("halo3", workgroups=6, k_slices=1),
          in_stride=96, out_stride=80, splitk=False, in_bn=True, in_relu=True,
          facts=dict(max_lines=3, crosses_depth=True, depth_taps=[2, 2], last_tile_rows=24, last_block_cols=8, partial_slab=16)),
    _same("halo3 half-N dgrad", 1, (1, 5, 70), K133, P011, 64, 40, _plan("halo3", cols=32, k_slices=1, workgroups=6), knobs=NO_DB_2,
          facts=dict(max_lines=3, last_tile_rows=94, last_half_cols=8)),
    _same("halo2 half-N KH1", 0, (1, 2, 130), K113, P001, 128, 64, _plan("halo2", cols=32, k_slices=1, workgroups=6), knobs=NO_DB_2,
          facts=dict(max_lines=2, last_tile_rows=4)),
    # more K slices than (kd, kh, slab) A tiles: the halo geometry runs on the plain kernel
    _same("slices beyond A tiles", 0, (1, 2, 130), K113, P001, 128, 64, _plan("igemm", k_slices=3, double_buffered=0),
          knobs=NO_DB_3, facts=dict(last_tile_rows=4)),
    _same("slices beyond A tiles db", 0, (1, 2, 130), K113, P001, 128, 64, _plan("igemm", k_slices=3, double_buffered=1),
          knobs=dict(force_splitk=3), facts=dict(last_tile_rows=4)),
    _same("small tile halo", 0, (1, 3, 70), K133, P011, 64, 64, _plan("halo2", tile_rows=64, k_slices=3, tiles=4),
          flags=("SMALL_TILE",), in_bn=True, in_relu=True, facts=dict(last_tile_rows_64=18)),
    _same("small tile halo, 128 rows", 0, (1, 3, 70), K133, P011, 64, 64, _plan("halo3", tile_rows=128, k_slices=3, tiles=2),
          in_bn=True, in_relu=True, like="small tile halo", facts=dict(last_tile_rows=82, max_lines=2)),
    _same("wide W126", 0, (1, 2, 126), K133, P011, 64, 128, _plan("wide", cols=128, k_slices=3), knobs=dict(wide_tile=1),
          in_bn=POS, in_relu=True, facts=dict(max_lines=2, last_tile_rows=124)),
    _same("wide W131 dgrad", 1, (1, 3, 131), K133, P011, 72, 256, _plan("wide", cols=128, k_slices=6), knobs=dict(wide_tile=1),
          facts=dict(max_lines=2, last_tile_rows=9, partial_slab=8)),
    _same("wide W131 dgrad, as halo2", 1, (1, 3, 131), K133, P011, 72, 256, _plan("halo2", cols=64), facts=dict(last_tile_rows=9)),
    _same("wide refuses Cout 132", 1, (1, 3, 131), K133, P011, 72, 132, _plan("halo2"), knobs=dict(wide_tile=1),
          facts=dict(last_block_cols=4)),
    # ---- parity classes ---------------------------------------------------------------------------------------------------------
    _case("parity one wave", 1, (1, 1, 32), (1, 2, 64), K133, S122, P011, 64, 64, _plan("igemm", parity_classes=1, tiles=4),
          facts=dict(class_rows=32, class_last_tile_rows=32)),
    # Wo / 2 = 33: the 32 rows of a wave wrap a line
    _case("parity wrap", 1, (1, 3, 33), (1, 6, 66), K133, S122, P011, 128, 64, _plan("igemm", parity_classes=1, tiles=4),
          facts=dict(class_rows=99, class_last_tile_rows=99)),
    _case("parity 2 rows", 1, (1, 2, 65), (1, 4, 130), K133, S122, P011, 64, 128, _plan("igemm", parity_classes=1, tiles=8),
          facts=dict(class_rows=130, class_last_tile_rows=2)),
    _case("parity 2 rows bwd sink", 1, (1, 2, 65), (1, 4, 130), K133, S122, P011, 64, 128,
          _plan("igemm", parity_classes=1, tiles=8), stats="bwd sink", bwd_relu=True, gate=True,
          facts=dict(class_rows=130, class_last_tile_rows=2)),
    _case("parity k2 s2", 1, (1, 2, 33), (1, 4, 66), K122, S122, P0, 64, 64, _plan("igemm", parity_classes=1, k_slices=1),
          facts=dict(class_rows=66, class_last_tile_rows=66)),
    _case("parity refused W62", 1, (1, 2, 31), (1, 4, 62), K133, S122, P011, 64, 64, _plan("igemm", parity_classes=0)),
    _case("parity refused table", 1, (1, 1, 32), (1, 2, 64), K133, S122, P011, 64, 64, _plan("igemm", parity_classes=0),
          stats="table"),
    # ---- plane pairs ----------------------------------------------------------------------------------------------------------
    _case("plane pairs halo3", 0, (4, 384, 64), (2, 384, 64), K313, S211, P101, 20, 256,
          _plan("halo3", plane_pair=1, workgroups=768, k_slices=1), facts=dict(depth_taps=[2, 3], max_lines=2, partial_slab=20)),
    _case("plane pairs transposed", 1, (2, 96, 128), (4, 96, 128), K313, S211, P101, 20, 256,
          _plan("halo2", plane_pair=1, workgroups=768), facts=dict(depth_taps=[1, 2, 1, 1], max_lines=1)),
    _case("plane pairs transposed, off", 1, (2, 96, 128), (4, 96, 128), K313, S211, P101, 20, 256,
          _plan("halo2", plane_pair=0, workgroups=1536), knobs=dict(plane_pair=0), like="plane pairs transposed",
          facts=dict(depth_taps=[1, 2, 1, 1])),
    # ---- whole rounds + a K-sliced tail ---------------------------------------------------------------------------------------
    _same("two launches halo2", 0, (1, 70, 126), K113, P001, 128, 768,
          _plan("halo2", launches=2, tail_tile0=64, k_slices=2, workgroups=888, tiles=69), facts=dict(last_tile_rows=116, max_lines=2)),
    _same("two launches plain", 0, (1, 140, 63), K113, P001, 128, 768,
          _plan("igemm", launches=2, tail_tile0=64, k_slices=2, workgroups=888, tiles=69), facts=dict(last_tile_rows=116, max_lines=4)),
    # ---- the resident Dense(64) kernel --------------------------------------------------------------------------------------------
    _same("dense64 threshold", 0, (1, 768, 128), K111, P0, 64, 64, _plan("dense64", workgroups=768, tiles=768)),
    _same("dense64 one tile short", 0, (1, 767, 128), K111, P0, 64, 64, _plan("igemm", workgroups=767, k_slices=1)),
    # ---- pixel-shuffle store: 6 x 10 positions x (2 x 2 taps x 256 channels) into channels 256 .. 511 of a 12 x 20 x 768 map ------
    _same("pixel shuffle", 0, (1, 6, 10), K111, P0, 128, 1024, _plan("igemm", workgroups=16, k_slices=1), out_stride=768, ps=2,
          ps_channels=256, in_bn=True, in_relu=True, facts=dict(last_tile_rows=60)),
]

ROWS_GEOM = (1, (4, 12, 20), (8, 12, 20), K333, S211, P111, 64, 64)
ROWS_CAPACITY, QUEUE_CAPACITY = 1000, 768 * 128
CASES += [
    # row list: tiles at or above the device count exit at once; count 128: the second tile starts AT the count
    _case(f"rows count {n}", *ROWS_GEOM, _plan("igemm", k_slices=9, tiles=8), rows=(ROWS_CAPACITY, n),
          facts=dict(live_tiles=-(-n // BM), last_live_tile_rows=n - (-(-n // BM) - 1) * BM if n else 0))
    for n in (0, 1, 128, 999)
] + [
    # tile queue: 768 resident workgroups draw tiles from a counter; tiles beyond the count are never drawn
    _case(f"queue count {n}", *ROWS_GEOM, _plan("queue", k_slices=1, workgroups=768, tiles=768), rows=(QUEUE_CAPACITY, n), queue=True,
          facts=dict(live_tiles=-(-n // BM), last_live_tile_rows=n - (-(-n // BM) - 1) * BM if n else 0))
    for n in (0, 129, QUEUE_CAPACITY - 1)
] + [
    # the same row list as one workgroup per tile: the same arithmetic
    _case("queue count 129, per tile", *ROWS_GEOM, _plan("igemm", k_slices=1, workgroups=768, tiles=768), rows=(QUEUE_CAPACITY, 129),
          like="queue count 129"),
]

# dense64, all five instantiations at 769 tiles.  768 * 128 + 1 = 5 * 19 661 has no factorisation into three dims below 1024;
# 199 * 494 = 768 * 128 + 2 is the nearest that has: the last tile holds TWO rows.
D64 = (1, 199, 494)
_D64_PLAN = _plan("dense64", workgroups=768, tiles=769, k_slices=1)
_D64_FACTS = dict(last_tile_rows=2)
CASES += [
    _same("dense64 forward bn relu", 0, D64, K111, P0, 64, 64, _D64_PLAN, in_bn=True, in_relu=True, out_relu=True, facts=_D64_FACTS),
    _same("dense64 forward raw", 0, D64, K111, P0, 64, 64, _D64_PLAN, bias=False, facts=_D64_FACTS),
    _same("dense64 backward sink", 0, D64, K111, P0, 64, 64, _D64_PLAN, bias=False, stats="bwd sink", bwd_relu=True, facts=_D64_FACTS),
    _same("dense64 backward sink xf", 0, D64, K111, P0, 64, 64, _D64_PLAN, bias=False, in_bn=True, stats="bwd sink",
          facts=_D64_FACTS),
    _same("dense64 dense_dw", 0, D64, K111, P0, 64, 64, dict(_D64_PLAN, workgroups=512), bias=False, stats="bwd sink", bwd_relu=True,
          dense_dw=True, facts=_D64_FACTS),
]

# ---- BatchNormalization backward on load (in_y): plain tile, halo2, halo3; 72 channels = one slab + 8 beside the constants ----
for _fold in ("relu", "linear"):
    CASES += [
        _same(f"fold plain {_fold}", 1, (1, 3, 43), K133, P011, 72, 64, _plan("igemm", k_slices=1), fold=_fold, in_stride=80,
              splitk=False, facts=dict(partial_slab=8, last_tile_rows=1)),
        _same(f"fold halo2 {_fold}", 1, (1, 3, 130), K133, P011, 72, 64, _plan("halo2", k_slices=1), fold=_fold, in_stride=80,
              splitk=False, facts=dict(partial_slab=8, last_tile_rows=6, max_lines=2)),
        _same(f"fold halo3 {_fold}", 1, (1, 5, 70), K133, P011, 64, 64, _plan("halo3", k_slices=3, double_buffered=1), fold=_fold,
              facts=dict(last_tile_rows=94, max_lines=3)),
    ]
CASES.append(_same("fold halo3 half-N", 1, (1, 5, 70), K133, P011, 64, 40, _plan("halo3", cols=32, k_slices=1), fold="relu",
                   knobs=NO_DB_2, facts=dict(last_half_cols=8)))

# ---- the Dense(64) tail on the two-line halo kernel -----------------------------------------------------------------------------
_TAIL = _plan("halo2", k_slices=1, cols=64, launches=1)
for _w, _rows in ((126, 122), (129, 3)):
    CASES += [
        _same(f"tail W{_w}", 1, (1, 3, _w), K133, P011, 64, 64, _TAIL, tail=True, gate=True,
              facts=dict(last_tile_rows=_rows, max_lines=2)),
        _same(f"tail W{_w} bwd sink", 1, (1, 3, _w), K133, P011, 64, 64, _TAIL, tail=True, gate=True, stats="bwd sink",
              facts=dict(last_tile_rows=_rows, max_lines=2)),
    ]
CASES += [
    # output depth 3 over a source of depth 1: plane 2 has no live tap -- out is exactly gate(0), tail_out exactly 0
    _case("tail dead plane", 1, (1, 3, 126), (3, 3, 126), K333, S211, P111, 64, 64, dict(_TAIL, plane_pair=0), tail=True, gate=True,
          stats="bwd sink", knobs=dict(plane_pair=0), facts=dict(depth_taps=[1, 1, 0])),
    # ---- a dead depth plane on the plain form and on a halo form: the stored value is gate(bias + previous) in fp32, exactly ----
    _case("dead plane plain", 1, (1, 5, 20), (3, 5, 20), K333, S211, P111, 64, 64, _plan("igemm", k_slices=1), bias=True,
          accumulate=True, gate=True, splitk=False, facts=dict(depth_taps=[1, 1, 0], crosses_depth=True)),
    _case("dead plane halo3", 1, (1, 2, 70), (3, 2, 70), K333, S211, P111, 64, 64, _plan("halo3", k_slices=1), bias=True,
          accumulate=True, gate=True, splitk=False, facts=dict(depth_taps=[1, 1, 0], crosses_depth=True, max_lines=3)),
    _case("dead plane halo3 sliced", 1, (1, 2, 70), (3, 2, 70), K333, S211, P111, 64, 64, _plan("halo3", double_buffered=1),
          bias=True, accumulate=True, gate=True, facts=dict(depth_taps=[1, 1, 0])),
]

# ---- the epilogue switches on one ragged case per kernel family -----------------------------------------------------------------
# family: (dims, cin, cout, strides, splitk, knobs, plan, per-tile table allowed, gate allowed)
FAMILIES = {
    "igemm": ((1, 3, 43), 68, 72, (72, 80), False, {}, _plan("igemm", cols=64, k_slices=1), True, True),
    "sliced": ((1, 3, 43), 68, 72, (72, 80), True, NO_DB_3, _plan("igemm", cols=64, k_slices=3, double_buffered=0), True, True),
    "halo2": ((1, 3, 130), 68, 72, (72, 80), False, {}, _plan("halo2", cols=64, k_slices=1), True, True),
    "halo3": ((1, 5, 70), 68, 72, (72, 80), False, {}, _plan("halo3", cols=64, k_slices=1), True, True),
    "half-N": ((1, 13, 25), 96, 40, (None, 48), True, NO_DB_2, _plan("igemm", cols=32, k_slices=1), True, True),
    "wide": ((1, 3, 131), 72, 200, (None, 208), True, dict(wide_tile=1), _plan("wide", cols=128), False, False),
}
for _fam, (_dims, _ci, _co, (_is, _os), _sk, _kn, _pl, _table, _gate) in FAMILIES.items():
    _kw = dict(in_stride=_is, out_stride=_os, splitk=_sk, knobs=_kn)
    CASES += [
        _same(f"{_fam}: bias accumulate gate relu sink", 0, _dims, K133, P011, _ci, _co, _pl, bias=True, accumulate=True, gate=_gate,
              out_relu=True, stats="sink", in_bn=True, in_relu=True, **_kw),
        _same(f"{_fam}: accumulate gate bwd sink relu", 1, _dims, K133, P011, _ci, _co, _pl, accumulate=True, gate=_gate,
              stats="bwd sink", bwd_relu=True, **_kw),
        _same(f"{_fam}: bwd sink", 1, _dims, K133, P011, _ci, _co, _pl, stats="bwd sink", **_kw),
    ]
    if _table:
        CASES += [
            _same(f"{_fam}: bias relu table", 0, _dims, K133, P011, _ci, _co, _pl, bias=True, out_relu=True, stats="table",
                  in_bn=True, in_relu=True, **_kw),
            _same(f"{_fam}: gate bwd table relu", 1, _dims, K133, P011, _ci, _co, _pl, gate=True, stats="bwd table", bwd_relu=True,
                  **_kw),
        ]

# Forms the code documents as the SAME arithmetic: their outputs are compared bit for bit.
IDENTICAL = [("queue count 129", "queue count 129, per tile"), ("plane pairs transposed", "plane pairs transposed, off"),
             ("small tile halo", "small tile halo, 128 rows")]
# Forms that only reorder the sum: each meets the same bounds against the same reference (every case does; listed so that the
# pairs stay in the table): half-N vs K slices, sliced vs one pass, wide vs halo2.
REORDERED = [("half-N 128", "lone slices"), ("halo W126 sliced", "halo W126"), ("wide W131 dgrad", "wide W131 dgrad, as halo2")]

# (kernel, cols, double_buffered, sliced, launches, plane_pair, parity_classes, tile_rows) the table must reach
REQUIRED = {
    ("igemm", 64, 0, 0, 1, 0, 0, 128), ("igemm", 64, 1, 1, 1, 0, 0, 128), ("igemm", 64, 0, 1, 1, 0, 0, 128),
    ("igemm", 32, 0, 0, 1, 0, 0, 128), ("igemm", 64, 0, 0, 1, 0, 1, 128), ("igemm", 64, 1, 1, 1, 0, 1, 128), ("igemm", 64, 0, 1, 2, 0, 0, 128),
    ("halo3", 64, 1, 1, 1, 0, 0, 128), ("halo3", 64, 0, 0, 1, 0, 0, 128), ("halo3", 32, 0, 0, 1, 0, 0, 128),
    ("halo3", 64, 0, 0, 1, 1, 0, 128),
    ("halo2", 64, 1, 1, 1, 0, 0, 128), ("halo2", 64, 0, 0, 1, 0, 0, 128), ("halo2", 32, 0, 0, 1, 0, 0, 128),
    ("halo2", 64, 0, 0, 1, 1, 0, 128), ("halo2", 64, 0, 1, 2, 0, 0, 128), ("halo2", 64, 1, 1, 1, 0, 0, 64),
    ("wide", 128, 0, 1, 1, 0, 0, 128), ("dense64", 64, 0, 0, 1, 0, 0, 128), ("queue", 64, 0, 0, 1, 0, 0, 128),
}


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def seed_of(name):
    return zlib.crc32(name.encode())


def operands_of(c):
    """the name that seeds the operands (and keys the reference) of a case"""
    return c["like"] or c["name"]


def form_of(plan):
    return (plan["kernel"], plan["cols"], plan["double_buffered"], int(plan["k_slices"] > 1), plan["launches"], plan["plane_pair"],
            plan["parity_classes"], plan["tile_rows"])


def geom_of(c):
    from lisec_amd import ops
    return ops.geom(c["mode"], c["ind"], c["outd"], c["k"], c["s"], c["p"], c["cin"], c["cout"], in_stride=c["in_stride"],
                    out_stride=c["out_stride"], ps=c["ps"], ps_channels=c["ps_channels"])


def flags_of(c):
    from lisec_amd import ops
    f = (ops.IN_RELU if c["in_relu"] else 0) | (ops.OUT_RELU if c["out_relu"] else 0) | (ops.ACCUMULATE if c["accumulate"] else 0)
    for name in c["flags"]:
        f |= getattr(ops, name)
    return f


def plan_of(c):
    """ops.conv_plan of the case on the host: the extras are present / absent as the call's will be (the planner only asks
    whether a pointer is NULL and how it is aligned)."""
    import torch
    from lisec_amd import ops
    g = geom_of(c)
    t = torch.zeros(8)                                   # any 16-byte aligned non-NULL pointer
    kw = {}
    stats = c["stats"] or ""
    if c["gate"]:
        kw["out_mask"] = t
    if stats.startswith("bwd"):
        kw["bwd"] = (t, t, c["bwd_relu"])
    if stats.endswith("sink"):
        cy = 64 if c["tail"] else c["cout"]
        M = int(np.prod(c["outd"]))
        kw["sink"] = (ops.BnSink(cy, M, "cpu", dgamma=t, dbeta=t) if stats.startswith("bwd") else
                      ops.BnSink(cy, M, "cpu", gamma=t, beta=t, bnstate=t))
    if c["queue"]:
        kw["queue"] = t
    if c["tail"]:
        kw["tail"] = (t, t)
    if c["fold"]:
        kw["fold"] = (t, t, t, c["fold"] == "relu")
    if c["dense_dw"]:
        kw["dense_dw"] = t
    return ops.conv_plan(g, in_bn=bool(c["in_bn"]), flags=flags_of(c), stats=stats.endswith("table"), splitk=c["splitk"],
                         rows_capacity=c["rows"][0] if c["rows"] else 0, **kw)


# ---- the geometric facts, from the dims alone -------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def facts_of(c):
    """What the geometry of a case gives, without the planner: rows in the last 128-row (and 64-row) tile; whether a tile
    crosses a depth boundary; the largest number of output lines a 128-row tile touches; rows per parity class and in each
    class's last tile; live depth taps per output plane; live columns of the last 64-column block and of the last 32-column
    half; the channels of a partial last slab (0: none); for a row list the tiles that hold rows and the rows of the last."""
    Do, Ho, Wo = c["outd"]
    M = Do * Ho * Wo
    f = dict(last_tile_rows=M - (_cdiv(M, BM) - 1) * BM, last_tile_rows_64=M - (_cdiv(M, 64) - 1) * 64)
    tiles = [(m0, min(m0 + BM, M) - 1) for m0 in range(0, M, BM)]
    f["crosses_depth"] = any(a // (Ho * Wo) != b // (Ho * Wo) for a, b in tiles)
    f["max_lines"] = max(b // Wo - a // Wo + 1 for a, b in tiles)
    if c["mode"] == 1 and c["s"] == S122 and Do == 1 and Ho % 2 == 0 and Wo % 2 == 0:
        rows = (Ho // 2) * (Wo // 2)
        f.update(class_rows=rows, class_last_tile_rows=rows - (_cdiv(rows, BM) - 1) * BM)
    f["depth_taps"] = [sum(source_plane(c["mode"], d, kd, c["s"][0], c["p"][0], c["ind"][0]) is not None for kd in range(c["k"][0]))
                       for d in range(Do)]
    f["last_block_cols"] = c["cout"] - (_cdiv(c["cout"], 64) - 1) * 64
    f["last_half_cols"] = c["cout"] - (_cdiv(c["cout"], 32) - 1) * 32
    f["partial_slab"] = c["cin"] % 64
    if c["rows"]:
        n = c["rows"][1]
        f.update(live_tiles=_cdiv(n, BM), last_live_tile_rows=n - (_cdiv(n, BM) - 1) * BM if n else 0)
    return f


# ---- operands ---------------------------------------------------------------------------------------------------------------------
GATE_MARGIN = 1e-4


def _away_from_zero(y, st, C):
    """y with every element whose BatchNormalization gate scale * y + shift lies within GATE_MARGIN of zero moved by
    1e-2 / scale: fp32 and fp64 then agree on which side of the gate it is."""
    scale, shift = st[:C].astype(np.float64), st[C:2 * C].astype(np.float64)
    near = np.abs(y.astype(np.float64) * scale + shift) < GATE_MARGIN
    return np.where(near, y + (1e-2 / scale).astype(np.float32), y).astype(np.float32)


def out_shape(c):
    """the tensor the call stores to: (planes, H, W), channels"""
    if c["rows"]:
        return (1, 1, c["rows"][0]), c["cout"]
    Do, Ho, Wo = c["outd"]
    if c["ps"]:
        return (Do, Ho * c["ps"], Wo * c["ps"]), c["ps_channels"]
    return (Do, Ho, Wo), c["cout"]


def draw(c):
    """The operands of a case, by name: x (*ind, cin), W (taps, cin, cout), and as the case asks: bias, in_bn (bnstate of the
    producing layer), prev (what ACCUMULATE adds onto), gate (with exact +0.0 and -0.0 entries), y / y_bn (raw output and bnstate
    of the BatchNormalization a gradient is about to cross; 64 columns with a tail), gamma / beta / moving_mean / moving_var,
    fold_y / fold_bn / fold_coef (x is then the gradient w.r.t. relu(bn(fold_y))), Wd (1, 64, 64) the tail kernel, coords
    (capacity, 3) the row list, sorted by cell."""
    rng = np.random.default_rng(seed_of(operands_of(c)))
    f32 = lambda a: a.astype(np.float32)
    taps, cin, cout = int(np.prod(c["k"])), c["cin"], c["cout"]
    o = dict(x=f32(rng.normal(0, 1, (*c["ind"], cin))), W=f32(rng.normal(0, 1, (taps, cin, cout)) / np.sqrt(taps * cin)))
    dims, ch = out_shape(c)
    if c["bias"]:
        o["bias"] = f32(rng.normal(0, 0.1, ch))
    if c["in_bn"]:
        o["in_bn"] = bn_state(rng, cin, None if c["in_bn"] is True else c["in_bn"])
    if c["accumulate"]:
        o["prev"] = f32(rng.normal(0, 1, (*dims, ch)))
    if c["gate"]:
        gate = f32(rng.normal(0, 1, (*dims, ch)))
        flat = gate.reshape(-1)
        flat[0::7] = np.float32(0.0)                     # the kernel's test is mask > 0: both zeros close the gate
        flat[3::7] = np.float32(-0.0)
        o["gate"] = gate
    stats = c["stats"] or ""
    if stats.startswith("bwd"):
        cy = 64 if c["tail"] else cout
        o["y_bn"] = bn_state(rng, cy)
        y = f32(rng.normal(0, 1, (*c["outd"], cy)))
        o["y"] = _away_from_zero(y, o["y_bn"], cy) if c["bwd_relu"] else y
    elif stats:
        o["gamma"], o["beta"] = f32(rng.uniform(0.5, 1.5, cout)), f32(rng.normal(0, 0.2, cout))
        if stats == "sink":
            o["moving_mean"], o["moving_var"] = f32(rng.normal(0, 0.2, cout)), f32(rng.uniform(0.5, 1.5, cout))
    if c["fold"]:
        o["fold_bn"] = st = bn_state(rng, cin)
        y = f32(rng.normal(0, 1, (*c["ind"], cin)))
        o["fold_y"] = y = _away_from_zero(y, st, cin) if c["fold"] == "relu" else y
        s64, y64 = st.astype(np.float64), y.astype(np.float64)
        dz = o["x"].astype(np.float64)
        if c["fold"] == "relu":
            dz = np.where(y64 * s64[:cin] + s64[cin:2 * cin] > 0, dz, 0.0)
        yhat = (y64 - s64[2 * cin:3 * cin]) * s64[3 * cin:]
        o["fold_coef"] = f32(np.concatenate([dz.reshape(-1, cin).mean(0), (dz * yhat).reshape(-1, cin).mean(0)]))
    if c["tail"]:
        o["Wd"] = f32(rng.normal(0, 1, (1, 64, 64)) / 8)
    if c["rows"]:
        Do, Ho, Wo = c["outd"]
        cells = np.sort(rng.integers(0, Do * Ho * Wo, c["rows"][0]))
        o["coords"] = np.stack([cells // (Ho * Wo), (cells // Wo) % Ho, cells % Wo], 1).astype(np.int32)
    return o


def gate_arguments(c, o):
    """the arguments scale * y + shift (fp64) of every BatchNormalization gate the case evaluates with a ReLU"""
    out = []
    if c["bwd_relu"] and "y" in o:
        C = o["y"].shape[-1]
        st = o["y_bn"].astype(np.float64)
        out.append(o["y"].astype(np.float64) * st[:C] + st[C:2 * C])
    if c["fold"] == "relu":
        C = c["cin"]
        st = o["fold_bn"].astype(np.float64)
        out.append(o["fold_y"].astype(np.float64) * st[:C] + st[C:2 * C])
    return out
