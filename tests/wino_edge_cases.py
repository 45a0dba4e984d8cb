"""Edge geometries of the Winograd F(2x2, 3x3) kernels (csrc/wino.hip: k_wino, k_wino_pack; csrc/wino_wgrad.hip: k_wino_wgrad,
k_wino_wgrad_sum, k_wino_wgrad_finish), shared by tests/test_wino_edge_cases.py (CPU: every case is served, and has the launch
structure it is listed for) and tests/test_gpu_wino_edges.py (the kernels against fp64) -- TEST ONLY.

A forward / data-gradient case (FWD) is a dict: name, mode, ind / outd (d, h, w), kd / sd / pd (depth taps, stride, pad; the
(h, w) taps are 3 x 3, stride 1, pad 1), cin, cout, in_stride / out_stride (None: dense), in_bn (None, True, or the (lo, hi)
range its shifts are drawn from; with in_bn the ReLU on load is on), bias, accumulate, out_relu, gate, sink (None, "fwd",
"fwd moving 1" / "fwd moving 0": moving statistics with unbiased 1 / 0, "bwd"), bwd_relu, tail (None, "net": gate + bwd_y +
backward sink as LisecNet calls it, "no gate", "plain": tail_out only), pack ("k-major", or "net": the data-gradient packing
of LisecNet._pack_transposed -- the forward layer's kernel read with k_stride 1, n_stride K) and facts.
A weight-gradient case (WGRAD) is a dict: name, ind, outd, kd, sd, pd (64 -> 64, mode 0, packed rows) and facts.

facts are the structural reasons a case is in the table; structure(case) / wgrad_structure(case, cus) restate the launch
structure FROM THE GEOMETRY (not from the library) and tests/test_wino_edge_cases.py asserts that the two agree.
Inputs are default_rng(crc32(name)) normals, float32; kernels are scaled by 1 / sqrt(taps * cin)."""
import zlib

import numpy as np

CUS = 256                     # compute units the weight-gradient facts are stated for (an MI355X; the library's host default)


def _fwd(name, mode, ind, outd, kd, sd, pd, cin, cout, facts, in_stride=None, out_stride=None, in_bn=None, bias=None,
         accumulate=False, out_relu=False, gate=False, sink=None, bwd_relu=False, tail=None, pack="k-major"):
    return dict(name=name, mode=mode, ind=ind, outd=outd, kd=kd, sd=sd, pd=pd, cin=cin, cout=cout, facts=facts,
                in_stride=in_stride, out_stride=out_stride, in_bn=in_bn, bias=(mode == 0) if bias is None else bias,
                accumulate=accumulate, out_relu=out_relu, gate=gate, sink=sink, bwd_relu=bwd_relu, tail=tail, pack=pack)


def _2d(name, mode, hw, cin, cout, facts, **kw):
    return _fwd(name, mode, (1, *hw), (1, *hw), 1, 1, 0, cin, cout, facts, **kw)


def _facts(BH, BW, nnb, interior, launches, chunks):
    """launches: [(live depth taps, gridDim.x)] in launch order; interior: [(by, bx)]; chunks: K chunks per depth tap"""
    return dict(BH=BH, BW=BW, nnb=nnb, interior=interior, launches=launches, chunks=chunks)


POS = (0.5, 1.5)              # shifts in (0.5, 1.5): padding that is not gated to exact zero turns positive
D610 = (6, 10)                # the map of the depth cases: one block per plane
NET = dict(tail="net", gate=True, sink="bwd", pack="net")

FWD = [
    # ---- map ladder: 2D, mode 0, 16 -> 64, bias, BN + ReLU on load with positive shifts ---------------------------------------
    _2d("map 2x2", 0, (2, 2), 16, 64, _facts(1, 1, 1, [], [(1, 1)], 2), in_bn=POS),
    _2d("map 2x3", 0, (2, 3), 16, 64, _facts(1, 1, 1, [], [(1, 1)], 2), in_bn=POS),
    _2d("map 3x2", 0, (3, 2), 16, 64, _facts(1, 1, 1, [], [(1, 1)], 2), in_bn=POS),
    _2d("map 15x17", 0, (15, 17), 16, 64, _facts(1, 2, 1, [], [(1, 2)], 2), in_bn=POS),
    # three blocks in a column, the last one row high; too narrow for an interior block
    _2d("map 33x9", 0, (33, 9), 16, 64, _facts(3, 1, 1, [], [(1, 3)], 2), in_bn=POS),
    # four blocks, none interior: the window of block (1, 1) ends on row 32, one past the map
    _2d("map 32x32", 0, (32, 32), 16, 64, _facts(2, 2, 1, [], [(1, 4)], 2), in_bn=POS),
    # nine blocks, exactly (1, 1) interior (its window ends on row / column 32, the last of the map); the last blocks hold one
    # row / one column
    _2d("map 33x33", 0, (33, 33), 16, 64, _facts(3, 3, 1, [(1, 1)], [(1, 9)], 2), in_bn=POS),
    _2d("map 48x50 mode 1", 1, (48, 50), 16, 64, _facts(3, 4, 1, [(1, 1), (1, 2)], [(1, 12)], 2)),
    # ---- the same pair without BatchNormalization on load: the XF = false instantiation -------------------------------------
    _2d("map 32x32 raw", 0, (32, 32), 16, 64, _facts(2, 2, 1, [], [(1, 4)], 2)),
    _2d("map 33x33 raw", 0, (33, 33), 16, 64, _facts(3, 3, 1, [(1, 1)], [(1, 9)], 2)),
    # ---- channels ---------------------------------------------------------------------------------------------------------
    # Cout 8: wave column 1 (channels 32..63) wholly outside, column 0 three quarters outside
    _2d("channels 16->8", 0, (33, 35), 16, 8, _facts(3, 3, 1, [(1, 1)], [(1, 9)], 2), in_bn=True),
    _2d("channels 32->33", 0, (33, 35), 32, 33, _facts(3, 3, 1, [(1, 1)], [(1, 9)], 4), in_bn=True),
    # four column blocks, the last holds 8 channels
    _2d("channels 48->200", 0, (33, 35), 48, 200, _facts(3, 3, 4, [(1, 1)], [(1, 9)], 6), in_bn=True),
    _2d("channels 256->256", 0, (18, 18), 256, 256, _facts(2, 2, 4, [], [(1, 4)], 32), in_bn=True),
    # ---- strided operands (17 x 19, mode 1) ------------------------------------------------------------------------------
    _2d("stride in 64/80", 1, (17, 19), 64, 64, _facts(2, 2, 1, [], [(1, 4)], 8), in_stride=80),
    _2d("stride out 64/96", 1, (17, 19), 64, 64, _facts(2, 2, 1, [], [(1, 4)], 8), out_stride=96, accumulate=True, gate=True,
        sink="bwd", bwd_relu=True),
    _2d("stride in 64/80 out 64/96", 1, (17, 19), 64, 64, _facts(2, 2, 1, [], [(1, 4)], 8), in_stride=80, out_stride=96,
        accumulate=True, gate=True, sink="bwd", bwd_relu=True),
    # ---- depth taps ---------------------------------------------------------------------------------------------------------
    _fwd("depth KD 2 valid", 0, (3, *D610), (2, *D610), 2, 1, 0, 16, 64, _facts(1, 1, 1, [], [(2, 2)], 2)),
    _fwd("depth KD 4 valid", 0, (5, *D610), (2, *D610), 4, 1, 0, 16, 64, _facts(1, 1, 1, [], [(4, 2)], 2), in_bn=True),
    # plane 0 reads planes -1..2 (kd 0 dead), plane 1 reads 1..4 (kd 3 dead): three live taps each, but not the same three
    _fwd("depth KD 4 stride 2 pad 1", 0, (4, *D610), (2, *D610), 4, 2, 1, 16, 64, _facts(1, 1, 1, [], [(3, 2)], 2)),
    # live taps per plane 1, 2, 2, 1: two launches
    _fwd("depth KD 4 stride 2 pad 1 mode 1", 1, (2, *D610), (4, *D610), 4, 2, 1, 16, 64,
         _facts(1, 1, 1, [], [(2, 2), (1, 2)], 2)),
    _fwd("depth KD 4 stride 2 pad 1 mode 1 33x34", 1, (2, 33, 34), (4, 33, 34), 4, 2, 1, 16, 64,
         _facts(3, 3, 1, [(1, 1)], [(2, 18), (1, 18)], 2)),
    # all eight nibbles of plane_list in one launch
    _fwd("depth KD 3 valid 10->8", 0, (10, *D610), (8, *D610), 3, 1, 0, 16, 64, _facts(1, 1, 1, [], [(3, 8)], 2)),
    # launches of 5 and 2 workgroups
    _fwd("depth KD 3 pad 1 7->7", 0, (7, *D610), (7, *D610), 3, 1, 1, 16, 64, _facts(1, 1, 1, [], [(3, 5), (2, 2)], 2)),
    # output planes 1 and 3 divide by no stride: a launch with ZERO taps, out = gate(bias + previous) exactly
    _fwd("depth dead planes sink", 1, (2, *D610), (4, *D610), 1, 2, 0, 16, 64, _facts(1, 1, 1, [], [(1, 2), (0, 2)], 2),
         bias=True, sink="fwd"),
    _fwd("depth dead planes accumulate", 1, (2, *D610), (4, *D610), 1, 2, 0, 16, 64,
         _facts(1, 1, 1, [], [(1, 2), (0, 2)], 2), bias=True, accumulate=True, gate=True),
    # ---- statistics on partial blocks and a partial column block ---------------------------------------------------------------
    _2d("sink fwd moving 1", 0, (33, 35), 16, 72, _facts(3, 3, 2, [(1, 1)], [(1, 9)], 2), in_bn=True, sink="fwd moving 1"),
    _2d("sink fwd moving 0", 0, (33, 35), 16, 72, _facts(3, 3, 2, [(1, 1)], [(1, 9)], 2), in_bn=True, sink="fwd moving 0"),
    _2d("sink fwd out_relu", 0, (33, 35), 16, 72, _facts(3, 3, 2, [(1, 1)], [(1, 9)], 2), in_bn=True, sink="fwd",
        out_relu=True),
    _2d("sink bwd accumulate gate", 1, (17, 19), 16, 40, _facts(2, 2, 1, [], [(1, 4)], 2), sink="bwd", bwd_relu=True,
        accumulate=True, gate=True),
    _2d("sink bwd no relu", 1, (17, 19), 16, 40, _facts(2, 2, 1, [], [(1, 4)], 2), sink="bwd", bwd_relu=False),
    # ---- the Dense(64) tail (64 -> 64, mode 1) ------------------------------------------------------------------------------
    _2d("tail 2x2 net", 1, (2, 2), 64, 64, _facts(1, 1, 1, [], [(1, 1)], 8), **NET),
    _2d("tail 33x35 net", 1, (33, 35), 64, 64, _facts(3, 3, 1, [(1, 1)], [(1, 9)], 8), **NET),
    # launches of unequal tap counts (live taps 1, 2, 2, 1) sharing ONE sink
    _fwd("tail depth net", 1, (2, 9, 11), (4, 9, 11), 3, 1, 0, 64, 64, _facts(1, 1, 1, [], [(2, 2), (1, 2)], 8), **NET),
    _2d("tail 33x35 no gate", 1, (33, 35), 64, 64, _facts(3, 3, 1, [(1, 1)], [(1, 9)], 8), tail="no gate", sink="bwd",
        bwd_relu=True),
    _2d("tail 2x2 plain", 1, (2, 2), 64, 64, _facts(1, 1, 1, [], [(1, 1)], 8), tail="plain"),
    _fwd("tail depth plain", 1, (2, 9, 11), (4, 9, 11), 3, 1, 0, 64, 64, _facts(1, 1, 1, [], [(2, 2), (1, 2)], 8),
         tail="plain", pack="net"),
]


def _wg(name, ind, outd, kd, sd, pd, facts):
    return dict(name=name, ind=ind, outd=outd, kd=kd, sd=sd, pd=pd, facts=facts)


def _wfacts(live, units, per_tap, largest, smallest):
    """live depth taps, units per live tap, and on CUS compute units: workgroups per tap, largest / smallest share of units"""
    return dict(live=live, units=units, per_tap=per_tap, largest=largest, smallest=smallest)


def _wg2d(hw, units):
    return _wg(f"wgrad {hw[0]}x{hw[1]}", (1, *hw), (1, *hw), 1, 1, 0, _wfacts([0], [units], 256, 1, 0))


WGRAD = [
    _wg2d((2, 2), 1),         # 7 of the unit's 8 chunks lie wholly outside the map
    _wg2d((3, 3), 1), _wg2d((2, 9), 1), _wg2d((9, 2), 1), _wg2d((5, 7), 1), _wg2d((16, 16), 1), _wg2d((17, 17), 4),
    _wg2d((33, 9), 3),
    _wg("wgrad KD 2 valid", (3, *D610), (2, *D610), 2, 1, 0, _wfacts([0, 1], [2, 2], 128, 1, 0)),
    _wg("wgrad KD 4 valid", (5, *D610), (2, *D610), 4, 1, 0, _wfacts([0, 1, 2, 3], [2, 2, 2, 2], 64, 1, 0)),
    _wg("wgrad KD 4 stride 2 pad 1", (4, *D610), (2, *D610), 4, 2, 1, _wfacts([0, 1, 2, 3], [1, 2, 2, 1], 64, 1, 0)),
    # taps kd 0 and kd 2 read no plane: their 18 kernel taps are exactly 0.0 and every workgroup serves kd 1
    _wg("wgrad dead taps", (1, *D610), (1, *D610), 3, 2, 1, _wfacts([1], [1], 256, 1, 0)),
    # 8 planes x 3 x 4 blocks = 96 units per tap on 85 workgroups: eleven own two units, the rest one
    _wg("wgrad uneven shares", (10, 48, 64), (8, 48, 64), 3, 1, 0, _wfacts([0, 1, 2], [96, 96, 96], 85, 2, 1)),
]


def fwd_by_name(name):
    return next(c for c in FWD if c["name"] == name)


def wgrad_by_name(name):
    return next(c for c in WGRAD if c["name"] == name)


def seed_of(name):
    return zlib.crc32(name.encode())


# ---- the launch structure, restated from the geometry -------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def source_plane(mode, d, kd, sd, pd, Di):
    """the input plane depth tap kd of output plane d reads, or None (outside the tensor / not on the stride's lattice)"""
    if mode == 0:
        s = d * sd - pd + kd
        return s if 0 <= s < Di else None
    t = d + pd - kd
    if t < 0 or t % sd:
        return None
    return t // sd if t // sd < Di else None


def blocks(H, W):
    """(BH, BW): a workgroup's block is 8 x 8 tiles of 2 x 2 outputs = 16 x 16 outputs"""
    return _cdiv(_cdiv(H, 2), 8), _cdiv(_cdiv(W, 2), 8)


def structure(c):
    """BH, BW, nnb, the interior blocks (the 18 x 18 input window of the block -- rows 16 by - 1 .. 16 by + 16 -- lies inside
    the map), live depth taps per output plane, the launches (one per distinct tap count, most taps first) with their
    gridDim.x, and the K chunks (8 input channels) per depth tap."""
    Do, H, W = c["outd"]
    BH, BW = blocks(H, W)
    inside = lambda b, n: 16 * b - 1 >= 0 and 16 * b + 16 <= n - 1
    interior = [(by, bx) for by in range(BH) for bx in range(BW) if inside(by, H) and inside(bx, W)]
    live = [sum(source_plane(c["mode"], d, kd, c["sd"], c["pd"], c["ind"][0]) is not None for kd in range(c["kd"]))
            for d in range(Do)]
    launches = [(t, live.count(t) * BH * BW) for t in sorted(set(live), reverse=True)]
    return dict(BH=BH, BW=BW, nnb=_cdiv(c["cout"], 64), interior=interior, live=live, launches=launches,
                chunks=c["cin"] // 8)


def wgrad_structure(c, cus=CUS):
    """live depth taps (some output plane reads a plane through them), units per live tap (planes x BH x BW), and for `cus`
    resident workgroups: workgroups per tap (the same for every tap) and the largest / smallest number of units one owns."""
    Do, H, W = c["outd"]
    BH, BW = blocks(H, W)
    planes = [sum(source_plane(0, d, kd, c["sd"], c["pd"], c["ind"][0]) is not None for d in range(Do)) for kd in range(c["kd"])]
    live = [kd for kd, n in enumerate(planes) if n]
    units = [planes[kd] * BH * BW for kd in live]
    per_tap = cus // len(live) if live else 0
    shares = [(_cdiv(u, per_tap), u // per_tap) for u in units]
    return dict(live=live, units=units, per_tap=per_tap, largest=max(s[0] for s in shares), smallest=min(s[1] for s in shares))


# ---- geometry and operands -----------------------------------------------------------------------------------------------
def geom_of(c, **over):
    from lisec_amd import ops
    f = dict(c, **over)
    return ops.geom(f.get("mode", 0), f["ind"], f["outd"], (f["kd"], 3, 3), (f["sd"], 1, 1), (f["pd"], 1, 1), f.get("cin", 64),
                    f.get("cout", 64), in_stride=f.get("in_stride"), out_stride=f.get("out_stride"))


def flags_of(c):
    from lisec_amd import ops
    return ((ops.IN_RELU if c["in_bn"] else 0) | (ops.ACCUMULATE if c["accumulate"] else 0) |
            (ops.OUT_RELU if c["out_relu"] else 0))


def bn_state(rng, c, shift_range=None):
    """bnstate float32[4C] {scale, shift, mean, invstd} of a producing layer (scale in [0.5, 1.5]; shift normal, or uniform
    in shift_range)"""
    scale = rng.uniform(0.5, 1.5, c)
    shift = rng.normal(0, 0.3, c) if shift_range is None else rng.uniform(*shift_range, c)
    return np.concatenate([scale, shift, rng.normal(0, 0.2, c), rng.uniform(0.7, 1.4, c)]).astype(np.float32)


def draw_fwd(c):
    """The operands of a forward / data-gradient case, by name: x (*ind, cin), W (taps, cin, cout), and as the case asks:
    bias, in_bn (bnstate of the producing layer), prev (what ACCUMULATE adds onto), gate, y / y_bn (raw output and bnstate of
    the BatchNormalization the gradient is about to cross; 64 columns with a tail), gamma / beta (+ moving_mean / moving_var),
    Wd (1, 64, 64): the tail kernel as the contraction sees it."""
    rng = np.random.default_rng(seed_of(c["name"]))
    f32 = lambda a: a.astype(np.float32)
    taps, cin, cout = c["kd"] * 9, c["cin"], c["cout"]
    o = dict(x=f32(rng.normal(0, 1, (*c["ind"], cin))), W=f32(rng.normal(0, 1, (taps, cin, cout)) / np.sqrt(taps * cin)))
    if c["bias"]:
        o["bias"] = f32(rng.normal(0, 0.1, cout))
    if c["in_bn"]:
        o["in_bn"] = bn_state(rng, cin, None if c["in_bn"] is True else c["in_bn"])
    if c["accumulate"]:
        o["prev"] = f32(rng.normal(0, 1, (*c["outd"], cout)))
    if c["gate"]:
        o["gate"] = f32(rng.normal(0, 1, (*c["outd"], cout)))
    if c["sink"] == "bwd":
        cy = 64 if c["tail"] else cout
        o["y"] = f32(rng.normal(0, 1, (*c["outd"], cy)))
        o["y_bn"] = bn_state(rng, cy)
    elif c["sink"]:
        o["gamma"], o["beta"] = f32(rng.uniform(0.5, 1.5, cout)), f32(rng.normal(0, 0.2, cout))
        if "moving" in c["sink"]:
            o["moving_mean"], o["moving_var"] = f32(rng.normal(0, 0.2, cout)), f32(rng.uniform(0.5, 1.5, cout))
    if c["tail"]:
        o["Wd"] = f32(rng.normal(0, 1, (1, 64, 64)) / 8)
    return o


def draw_wgrad(c):
    rng = np.random.default_rng(seed_of(c["name"]))
    return (rng.normal(0, 1, (*c["ind"], 64)).astype(np.float32), rng.normal(0, 1, (*c["outd"], 64)).astype(np.float32))
