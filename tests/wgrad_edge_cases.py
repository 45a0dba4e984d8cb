"""Weight-gradient geometries at the edges of plan_wgrad (csrc/wgrad.hip), shared by tests/test_wgrad_edge_plans.py (CPU: every
case engages the plan it is listed for) and tests/test_gpu_wgrad_edges.py (the kernels against fp64) -- TEST ONLY.

A case is a dict: name, mode, ind / outd / k / s / p (3-tuples d, h, w), cin, cout, in_stride / out_stride (None: dense),
in_bn (None, True, or the (lo, hi) range its shifts are drawn from), relu, transpose_out, knobs (lisec_tuning fields to set
for the call), plan (the fields of ops.wgrad_plan the case MUST give), and for the two special forms dy_bn (the dY operand
is transformed: scale/shift + ReLU on load) and rows = (capacity, device count) of a row list.
Inputs are default_rng(crc32(name)) normals, float32."""
import contextlib
import zlib

import numpy as np

K133, K113, K333, K111 = (1, 3, 3), (1, 1, 3), (3, 3, 3), (1, 1, 1)
S1 = (1, 1, 1)


def _case(name, mode, ind, outd, k, s, p, cin, cout, plan, in_stride=None, out_stride=None, in_bn=None, relu=False,
          transpose_out=False, knobs=None, dy_bn=False, rows=None):
    return dict(name=name, mode=mode, ind=ind, outd=outd, k=k, s=s, p=p, cin=cin, cout=cout, in_stride=in_stride,
                out_stride=out_stride, in_bn=in_bn, relu=relu, transpose_out=transpose_out, knobs=knobs or {}, plan=plan,
                dy_bn=dy_bn, rows=rows)


RING, HALO, PLAIN = dict(ring=1, halo=0), dict(ring=0, halo=1), dict(ring=0, halo=0)
IN_KERNEL = dict(combine_in_kernel=1, lane_reduce=0)
LANES = dict(combine_in_kernel=0, lane_reduce=1)            # RING_SUM on a ring plan, LANE_SUM otherwise
SLAB_SUM = dict(combine_in_kernel=0, lane_reduce=0)
R4_GEOM = (0, (2, 6, 12), (1, 6, 12), K333, (2, 1, 1), (1, 1, 1), 64, 64)
P1_GEOM = (0, (1, 9, 13), (1, 5, 7), K133, (1, 2, 2), (0, 1, 1), 20, 12)
P6_GEOM = (1, (2, 6, 10), (4, 6, 10), K333, (2, 1, 1), (1, 1, 1), 64, 64)
P6_CAPACITY = 300

CASES = [
    # ---- ring -----------------------------------------------------------------------------------------------------------
    # len 9: one full and one partial 8-row chunk; one partial channel block on either side
    _case("R1", 0, (1, 5, 9), (1, 5, 9), K133, S1, (0, 1, 1), 16, 20,
          dict(RING, **IN_KERNEL, mirrored=0, staging_passes=3, tile_rows=9, groups=1)),
    # two tiles per line of 66 and 65 rows, gy = gz = 2 with 16- and 8-channel tail blocks, strided operands
    _case("R2", 0, (1, 4, 131), (1, 4, 131), K133, S1, (0, 1, 1), 80, 72,
          dict(RING, **IN_KERNEL, staging_passes=5, tile_rows=66, tiles=8), in_stride=96, out_stride=80, in_bn=True, relu=True),
    # DR 128, len % 8 != 0; ReLU without an affine
    _case("R3", 0, (1, 3, 121), (1, 3, 121), K133, S1, (0, 1, 1), 64, 64,
          dict(RING, **IN_KERNEL, staging_passes=6, tile_rows=121), relu=True),
    # two (kd, d) pairs; kd = 0 reads no plane: kd_slices[0] = 0, taps 0..8 are exact zeros of k_wgrad_ring_reduce
    _case("R4", *R4_GEOM, dict(RING, **LANES, groups=2, staging_passes=3, tile_rows=12)),
    # 40 slices per cell (> wgrad_combine_max): k_wgrad_ring_reduce runs its 4-deep loop and its tail loop
    _case("R5", 0, (1, 40, 8), (1, 40, 8), K133, S1, (0, 1, 1), 64, 64,
          dict(RING, **LANES, slabs=40, runs_per_column=40, lines_per_run=1, tile_rows=8)),
    # runs of 2, 2 and 3 lines
    _case("R6", 0, (1, 7, 10), (1, 7, 10), K133, S1, (0, 1, 1), 64, 64,
          dict(RING, **IN_KERNEL, runs_per_column=3, lines_per_run=3, slabs=3), knobs=dict(wgrad_ring_slots=3)),
    # one line: kh = 0 and kh = 2 read none; every shift > 0, so the affine + ReLU makes the zero padding positive
    _case("R7", 0, (1, 1, 8), (1, 1, 8), K133, S1, (0, 1, 1), 64, 64,
          dict(RING, **IN_KERNEL, runs_per_column=1, lines_per_run=1, tile_rows=8, staging_passes=3), in_bn=(0.5, 1.5),
          relu=True),
    _case("R8 pad 0", 0, (1, 6, 11), (1, 4, 9), K133, S1, (0, 0, 0), 64, 64, dict(RING, **IN_KERNEL, tile_rows=9)),
    _case("R8 pad 2", 0, (1, 4, 8), (1, 6, 10), K133, S1, (0, 2, 2), 64, 64, dict(RING, **IN_KERNEL, tile_rows=10)),
    # mirrored ring, transposed store with a Cin tail
    _case("R9", 1, (1, 7, 12), (1, 5, 10), K133, S1, (0, 2, 2), 24, 36,
          dict(RING, **IN_KERNEL, mirrored=1, staging_passes=3), in_bn=True, relu=True, transpose_out=True),
    # ---- w-halo ---------------------------------------------------------------------------------------------------------
    # KH = 1: the halo kernel without a knob.  LT 108 -> DR 112: the A image has 114 rows, more than 7 passes stage
    _case("H1", 0, (1, 5, 108), (1, 5, 108), K113, S1, (0, 0, 1), 64, 64,
          dict(HALO, **IN_KERNEL, tile_rows=108, staging_passes=9, groups=1, slabs=5)),
    _case("H1 bn", 0, (1, 5, 108), (1, 5, 108), K113, S1, (0, 0, 1), 64, 64,
          dict(HALO, **IN_KERNEL, tile_rows=108, staging_passes=9, groups=1, slabs=5), in_bn=True, relu=True),
    # stride 2 along h: source line 2h - 1 + kh
    _case("H2", 0, (1, 9, 20), (1, 5, 20), K133, (1, 2, 1), (0, 1, 1), 32, 16,
          dict(HALO, **IN_KERNEL, staging_passes=7, groups=3, tile_rows=20)),
    _case("H3", 0, (1, 3, 127), (1, 3, 127), K113, S1, (0, 0, 1), 64, 64,
          dict(HALO, **IN_KERNEL, staging_passes=9, tile_rows=127)),
    # 17 (kd, d) pairs: the ring refuses
    _case("H4", 0, (12, 3, 12), (6, 3, 12), K333, (2, 1, 1), (1, 1, 1), 16, 16,
          dict(HALO, **IN_KERNEL, staging_passes=7, groups=9, tiles=18)),
    # groups that read nothing: zeros written by the combining kernel / by the two slab sums (dead_taps)
    _case("H5", *R4_GEOM, dict(HALO, **IN_KERNEL, groups=9, slabs=6), knobs=dict(wgrad_ring=0)),
    _case("H5b", *R4_GEOM, dict(HALO, **SLAB_SUM, groups=6, slabs=6), knobs=dict(wgrad_ring=0, wgrad_combine_max=0)),
    _case("H6", 0, (2, 40, 12), (1, 40, 12), K333, (2, 1, 1), (1, 1, 1), 64, 64,
          dict(HALO, **LANES, groups=6, slabs=40), knobs=dict(wgrad_ring=0)),
    # mirrored + dead (kd, kh) groups.  H7: kh = 0 and kh = 2 dead (symmetric under the mirror); H7 pad 0: only the
    # forward kh' = 2 is live, i.e. the taps 0..2 -- the mirror of the dead groups is NOT the dead groups themselves
    _case("H7", 1, (1, 1, 40), (1, 1, 40), K133, S1, (0, 1, 1), 64, 64,
          dict(HALO, **SLAB_SUM, mirrored=1, groups=1, slabs=1), transpose_out=True,
          knobs=dict(wgrad_ring=0, wgrad_combine_max=0)),
    _case("H7 pad 0", 1, (1, 1, 40), (1, 1, 40), K133, S1, (0, 0, 1), 64, 64,
          dict(HALO, **SLAB_SUM, mirrored=1, groups=1, slabs=1), transpose_out=True,
          knobs=dict(wgrad_ring=0, wgrad_combine_max=0)),
    # 14 tiles in slabs of 3, 3, 3, 3, 2 that cross line ends
    _case("H8", 0, (1, 7, 140), (1, 7, 140), K113, S1, (0, 0, 1), 64, 64,
          dict(HALO, **IN_KERNEL, tile_rows=70, tiles=14, slabs=5, tiles_per_slab=3, staging_passes=7),
          knobs=dict(wgrad_blocks=6)),
    # ---- plain ----------------------------------------------------------------------------------------------------------
    _case("P1", *P1_GEOM, dict(PLAIN, **SLAB_SUM, tiles=1, slabs=1, taps_per_group=3, groups=3, staging_passes=8)),
    # M = 129: the second tile holds one row
    _case("P2", 0, (1, 3, 43), (1, 3, 43), K111, S1, (0, 0, 0), 64, 64,
          dict(PLAIN, **SLAB_SUM, tiles=2, slabs=2, tiles_per_slab=1, taps_per_group=1), in_bn=True),
    _case("P3", 0, (1, 48, 96), (1, 48, 96), K111, S1, (0, 0, 0), 16, 16, dict(PLAIN, **LANES, tiles=36, slabs=36),
          transpose_out=True),
    # one tile spanning two depths: tile_live must not skip it for any kd
    _case("P4", 0, (4, 6, 10), (2, 3, 5), K333, (2, 2, 2), (1, 1, 1), 64, 64,
          dict(PLAIN, **SLAB_SUM, tiles=1, slabs=1, groups=9, taps_per_group=3)),
    # the dY operand transformed on load (the kernel == stride Conv2DTranspose gradient with swapped roles), Cout tail
    _case("P5", *P1_GEOM, dict(PLAIN, **SLAB_SUM, tiles=1, slabs=1, taps_per_group=3), dy_bn=True),
] + [
    # row list: tiles at or above the device count hold nothing; count 0 gives exact zeros
    _case(f"P6 count {n}", *P6_GEOM, dict(PLAIN, **SLAB_SUM, tiles=3, slabs=3, groups=9, taps_per_group=3),
          transpose_out=True, rows=(P6_CAPACITY, n)) for n in (0, 1, 128, 263)
]

# The (kind, staging passes) pairs and the reduce forms the table must reach between its cases.
REQUIRED_KERNELS = {("ring", 3), ("ring", 5), ("ring", 6), ("halo", 7), ("halo", 9), ("plain", 8)}
REQUIRED_REDUCES = {"in-kernel", "RING_SUM", "LANE_SUM", "SLAB_SUM"}

_RPN = dict(mode=0, k=K133, s=S1, p=(0, 1, 1), in_bn=True, relu=True)
B1_ITEMS = [dict(_RPN, ind=(1, 12, 40), outd=(1, 12, 40), cin=64, cout=64),
            dict(_RPN, ind=(1, 6, 20), outd=(1, 6, 20), cin=128, cout=64),
            dict(_RPN, ind=(1, 9, 33), outd=(1, 9, 33), cin=64, cout=128)]
# name, items (the keys of a case that an item of ops.WgradBatch has), knobs, the plan EVERY item must give when planned alone
BATCHES = [
    ("B1", B1_ITEMS, {}, dict(RING, staging_passes=3)),
    ("B2", B1_ITEMS, dict(wgrad_ring=0), dict(HALO, staging_passes=7)),
    # staging variants differ (ring 3 / 5 passes; as halo items one transforms on load and one does not): one by one
    ("B3", [c for c in CASES if c["name"] in ("R1", "R2")], {}, dict(RING)),
]


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


def seed_of(name):
    return zlib.crc32(name.encode())


def geom_of(c):
    from lisec_amd import ops
    return ops.geom(c["mode"], c["ind"], c["outd"], c["k"], c["s"], c["p"], c["cin"], c["cout"],
                    in_stride=c.get("in_stride"), out_stride=c.get("out_stride"))


def flags_of(c):
    from lisec_amd import ops
    return (ops.IN_RELU if c.get("relu") else 0) | (ops.DY_RELU if c.get("dy_bn") else 0)


def plan_of(c):
    from lisec_amd import ops
    return ops.wgrad_plan(geom_of(c), flags=flags_of(c), dy_bn=bool(c.get("dy_bn")),
                          rows_capacity=c["rows"][0] if c.get("rows") else 0)


def kernel_and_reduce(plan):
    """(kind, staging passes), reduce form of a plan"""
    kind = "ring" if plan["ring"] else "halo" if plan["halo"] else "plain"
    if plan["combine_in_kernel"]:
        reduce = "in-kernel"
    elif plan["lane_reduce"]:
        reduce = "RING_SUM" if plan["ring"] else "LANE_SUM"
    else:
        reduce = "SLAB_SUM"
    return (kind, plan["staging_passes"]), reduce


@contextlib.contextmanager
def tuning(**knobs):
    """The library's launch-plan knobs set for the block and put back after it."""
    from lisec_amd import _lib
    prev = _lib.set_tuning(**knobs) if knobs else {}
    try:
        yield
    finally:
        if prev:
            _lib.set_tuning(**prev)


def bn_state(rng, c, shift_range=None):
    """bnstate float32[4C] {scale, shift, mean, invstd} of a producing layer (scale in [0.5, 1.5]; shift normal, or uniform
    in shift_range)"""
    scale = rng.uniform(0.5, 1.5, c)
    shift = rng.normal(0, 0.3, c) if shift_range is None else rng.uniform(*shift_range, c)
    return np.concatenate([scale, shift, rng.normal(0, 0.2, c), rng.uniform(0.7, 1.4, c)]).astype(np.float32)


def draw(c, name=None):
    """The operands of a case or batch item: x (*ind, cin), dy (*outd, cout) -- (capacity, cout) for a row list --, the
    bnstate of the operand that is transformed on load (or None), and for a row list coords (capacity, 3), sorted by cell."""
    rng = np.random.default_rng(seed_of(name or c["name"]))
    x = rng.normal(0, 1, (*c["ind"], c["cin"])).astype(np.float32)
    rows = c.get("rows")
    dy = rng.normal(0, 1, (rows[0], c["cout"]) if rows else (*c["outd"], c["cout"])).astype(np.float32)
    st = None
    if c.get("in_bn"):
        st = bn_state(rng, c["cin"], None if c["in_bn"] is True else c["in_bn"])
    elif c.get("dy_bn"):
        st = bn_state(rng, c["cout"])
    coords = None
    if rows:
        Do, Ho, Wo = c["outd"]
        cells = np.sort(rng.integers(0, Do * Ho * Wo, rows[0]))
        coords = np.stack([cells // (Ho * Wo), (cells // Wo) % Ho, cells % Wo], 1).astype(np.int32)
    return x, dy, st, coords
