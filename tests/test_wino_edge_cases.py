"""Keeps tests/wino_edge_cases.py honest, on the host: every case is served by the Winograd entry points
(lisec_conv_winograd_supported / lisec_conv_wgrad_winograd_supported answer without a device), every case's listed facts equal
the launch structure restated from its geometry, between them the cases reach every structural edge the table exists for,
every case the table must hold is there, and the geometries the kernels do not serve are refused.
tests/test_gpu_wino_edges.py runs the same table on the GPU."""
import pytest
import torch

import wino_edge_cases as E

IDS_F = [c["name"] for c in E.FWD]
IDS_W = [c["name"] for c in E.WGRAD]


def extras_of(c, device="cpu"):
    """The keyword arguments (in_bn, flags, out_mask, bwd, sink, tail) ops.winograd_supported takes for a case; the tensors
    only have to exist."""
    from lisec_amd import ops
    z = lambda n: torch.zeros(n, device=device)
    cout = c["cout"]
    kw = dict(in_bn=bool(c["in_bn"]), flags=E.flags_of(c))
    if c["gate"]:
        kw["out_mask"] = z(4)
    if c["sink"] == "bwd":
        kw["bwd"] = (z(4), z(4), c["bwd_relu"])
        kw["sink"] = ops.BnSink(cout, 1, device, dgamma=z(cout), dbeta=z(cout))
    elif c["sink"]:
        kw["sink"] = ops.BnSink(cout, 1, device, gamma=z(cout), beta=z(cout), bnstate=z(4 * cout))
    if c["tail"]:
        kw["tail"] = (z(4096), z(4))
    return kw


@pytest.mark.parametrize("case", E.FWD, ids=IDS_F)
def test_forward_case_is_served_and_has_its_structure(case):
    from lisec_amd import ops
    assert ops.winograd_supported(E.geom_of(case), **extras_of(case)), case["name"]
    s = E.structure(case)
    got = {k: s[k] for k in case["facts"]}
    assert got == case["facts"], f"{case['name']}: restated {got}, listed {case['facts']}"


@pytest.mark.parametrize("case", E.WGRAD, ids=IDS_W)
def test_weight_gradient_case_is_served_and_has_its_structure(case):
    from lisec_amd import ops
    g = E.geom_of(case)
    assert ops.wgrad_winograd_supported(g), case["name"]
    s = E.wgrad_structure(case)
    assert s == case["facts"], f"{case['name']}: restated {s}, listed {case['facts']}"
    # the workspace the library asks for on 256 compute units: one slab per resident workgroup and one sum per live tap
    nkd = len(s["live"])
    assert ops.wgrad_winograd_workspace_bytes(g) == (E.CUS // nkd * nkd + nkd) * 16 * 64 * 64 * 4


def test_names_are_unique():
    assert len(set(IDS_F)) == len(IDS_F) and len(set(IDS_W)) == len(IDS_W)


def _all():
    return [(c, E.structure(c)) for c in E.FWD]


def test_the_table_reaches_every_forward_edge():
    cs = _all()

    def some(what, pred):
        hits = [c["name"] for c, s in cs if pred(c, s)]
        print(f"{what}: {hits}")
        assert hits, f"no case reaches: {what}"

    gated_neighbours = lambda s: s["interior"] and len(s["interior"]) < s["BH"] * s["BW"]
    some("an interior block next to gated ones, BN on load", lambda c, s: gated_neighbours(s) and c["in_bn"])
    some("an interior block next to gated ones, raw input", lambda c, s: gated_neighbours(s) and not c["in_bn"])
    for xf in (True, False):
        some(f"H = 32: four blocks, none interior (BN on load: {xf})",
             lambda c, s: c["outd"][1] == 32 and s["BH"] * s["BW"] == 4 and not s["interior"] and bool(c["in_bn"]) == xf)
        some(f"H = 33: exactly block (1, 1) interior (BN on load: {xf})",
             lambda c, s: c["outd"][1:] == (33, 33) and s["interior"] == [(1, 1)] and bool(c["in_bn"]) == xf)
    some("two interior blocks", lambda c, s: len(s["interior"]) == 2)
    for kd in (1, 2, 3, 4):
        some(f"KD {kd}", lambda c, s: c["kd"] == kd)
    some("KD 4 in mode 1", lambda c, s: c["kd"] == 4 and c["mode"] == 1)
    some("a launch with zero taps feeding a sink", lambda c, s: s["launches"][-1][0] == 0 and c["sink"])
    some("a launch with zero taps, accumulate + gate", lambda c, s: s["launches"][-1][0] == 0 and c["accumulate"] and c["gate"])
    some("eight plane slots in one launch", lambda c, s: c["outd"][0] == 8 and len(s["launches"]) == 1)
    some("launches of unequal tap counts and an interior block", lambda c, s: len(s["launches"]) == 2 and s["interior"])
    some("launches of unequal tap counts sharing one sink with a tail",
         lambda c, s: len(s["launches"]) == 2 and c["tail"] == "net")
    grids = {n for _, s in cs for _, n in s["launches"]}
    print("gridDim.x reached:", sorted(grids))
    assert {1, 2, 3, 5, 9} <= grids, sorted(grids)
    assert {1, 4} <= {s["nnb"] for _, s in cs}
    assert {2, 4, 6, 8, 32} <= {s["chunks"] for _, s in cs}
    some("a partial last column block", lambda c, s: s["nnb"] > 1 and c["cout"] % 64)
    some("Cout < 32", lambda c, s: c["cout"] < 32)
    some("the smallest map", lambda c, s: c["outd"][1:] == (2, 2) and not c["tail"])
    some("in_stride > Cin alone", lambda c, s: c["in_stride"] and not c["out_stride"])
    some("out_stride > Cout with accumulate, gate and a backward sink",
         lambda c, s: c["out_stride"] and not c["in_stride"] and c["accumulate"] and c["gate"] and c["sink"] == "bwd")
    some("both strides", lambda c, s: c["in_stride"] and c["out_stride"])
    for unbiased in (0, 1):
        some(f"forward sink, moving statistics, unbiased {unbiased}, partial blocks and column block",
             lambda c, s: c["sink"] == f"fwd moving {unbiased}" and c["cout"] % 64 and c["outd"][1] % 16)
    some("forward sink + OUT_RELU", lambda c, s: c["sink"] == "fwd" and c["out_relu"])
    some("backward sink + accumulate + gate, ReLU", lambda c, s: c["sink"] == "bwd" and c["accumulate"] and c["gate"]
         and c["bwd_relu"] and not c["tail"] and not c["out_stride"])
    some("backward sink without ReLU outside the tail", lambda c, s: c["sink"] == "bwd" and not c["bwd_relu"] and not c["tail"])
    for kind in ("net", "no gate", "plain"):
        some(f"tail: {kind}", lambda c, s: c["tail"] == kind)
    some("tail at 2 x 2", lambda c, s: c["tail"] and c["outd"][1:] == (2, 2))
    some("tail with an interior block", lambda c, s: c["tail"] and s["interior"])
    some("the network's data-gradient packing", lambda c, s: c["pack"] == "net")


def test_the_table_reaches_every_weight_gradient_edge():
    ws = [(c, E.wgrad_structure(c)) for c in E.WGRAD]
    assert {1, 2, 3, 4} <= {c["kd"] for c, _ in ws}
    dead = [c["name"] for c, s in ws if len(s["live"]) < c["kd"]]
    uneven = [c["name"] for c, s in ws if s["largest"] >= 2 and s["smallest"] >= 1 and s["largest"] != s["smallest"]]
    idle = [c["name"] for c, s in ws if s["smallest"] == 0]
    unequal = [c["name"] for c, s in ws if len(set(s["units"])) > 1]
    print(f"dead taps: {dead}; uneven multi-unit shares: {uneven}; workgroups without a unit: {idle}; unequal taps: {unequal}")
    assert dead and uneven and idle and unequal
    c = E.wgrad_by_name("wgrad dead taps")
    s = E.wgrad_structure(c)
    assert s["live"] == [1] and s["per_tap"] == E.CUS          # every workgroup serves kd 1
    c = E.wgrad_by_name("wgrad uneven shares")
    s = E.wgrad_structure(c)
    assert s["units"] == [96] * 3 and s["per_tap"] == 85 and 96 - 85 == 11


# Every case the table must hold, one line each: dropping a case from the table fails here.  (mode, (h, w), kd, cin, cout)
# and the properties that tell it from its neighbours.
REQUIRED_FWD = [
    *[dict(mode=0, hw=hw, cin=16, cout=64, in_bn=E.POS, bias=True) for hw in ((2, 2), (2, 3), (3, 2), (15, 17), (32, 32), (33, 33))],
    dict(mode=1, hw=(48, 50), cin=16, cout=64, in_bn=None),
    dict(mode=0, hw=(32, 32), in_bn=None), dict(mode=0, hw=(33, 33), in_bn=None),
    dict(hw=(33, 35), cin=16, cout=8), dict(hw=(33, 35), cin=32, cout=33), dict(hw=(33, 35), cin=48, cout=200),
    dict(hw=(18, 18), cin=256, cout=256),
    dict(mode=1, hw=(17, 19), cin=64, in_stride=80, out_stride=None),
    dict(mode=1, hw=(17, 19), cout=64, in_stride=None, out_stride=96, accumulate=True, gate=True, sink="bwd"),
    dict(mode=1, hw=(17, 19), in_stride=80, out_stride=96, accumulate=True, gate=True, sink="bwd"),
    dict(mode=0, hw=E.D610, kd=2, sd=1, pd=0, planes=(3, 2)), dict(mode=0, hw=E.D610, kd=4, sd=1, pd=0, planes=(5, 2)),
    dict(mode=0, hw=E.D610, kd=4, sd=2, pd=1, planes=(4, 2)), dict(mode=1, hw=E.D610, kd=4, sd=2, pd=1, planes=(2, 4)),
    dict(mode=1, hw=(33, 34), kd=4, sd=2, pd=1, planes=(2, 4)),
    dict(mode=0, hw=E.D610, kd=3, sd=1, pd=0, planes=(10, 8)),
    dict(mode=1, hw=E.D610, kd=1, sd=2, pd=0, planes=(2, 4), sink="fwd"),
    dict(mode=1, hw=E.D610, kd=1, sd=2, pd=0, planes=(2, 4), accumulate=True, gate=True),
    dict(hw=(33, 35), cout=72, sink="fwd moving 1", in_bn=True), dict(hw=(33, 35), cout=72, sink="fwd moving 0", in_bn=True),
    dict(sink="fwd", out_relu=True),
    dict(mode=1, hw=(17, 19), cout=40, sink="bwd", bwd_relu=True, accumulate=True, gate=True),
    dict(sink="bwd", bwd_relu=False, tail=None),
    dict(tail="net", hw=(2, 2)), dict(tail="net", hw=(33, 35)), dict(tail="net", hw=(9, 11), kd=3, planes=(2, 4)),
    dict(tail="no gate", gate=False, sink="bwd"), dict(tail="plain", sink=None, gate=False, hw=(2, 2)),
    dict(tail="plain", kd=3),
]
REQUIRED_WGRAD = [
    *[dict(hw=hw, kd=1) for hw in ((2, 2), (3, 3), (2, 9), (9, 2), (5, 7), (16, 16), (17, 17), (33, 9))],
    dict(kd=2, sd=1, pd=0, planes=(3, 2)), dict(kd=4, sd=1, pd=0, planes=(5, 2)), dict(kd=4, sd=2, pd=1, planes=(4, 2)),
    dict(kd=3, sd=2, pd=1, planes=(1, 1)), dict(kd=3, sd=1, pd=0, planes=(10, 8), hw=(48, 64)),
]


def _matches(c, need):
    view = dict(c, hw=tuple(c["outd"][1:]), planes=(c["ind"][0], c["outd"][0]))
    return all(view[k] == v for k, v in need.items())


@pytest.mark.parametrize("table,required", [(E.FWD, REQUIRED_FWD), (E.WGRAD, REQUIRED_WGRAD)], ids=["forward", "wgrad"])
def test_every_required_case_is_in_the_table(table, required):
    used = set()
    for need in required:
        hits = [c["name"] for c in table if _matches(c, need) and c["name"] not in used]
        assert hits, f"no case left for {need}"
        used.add(hits[0])                              # one case answers one requirement
    for c in table:                                    # the size limit of the suite: 48 x 64 x 8 planes
        d, h, w = c["outd"]
        assert h <= 48 and w <= 64 and d <= 8 and h * w * d <= 48 * 64 * 8, c["name"]


def test_refusals():
    """What wino_ok / wgrad_wino_ok turn away answers 0 from the `supported` calls."""
    from lisec_amd import ops
    z = lambda n: torch.zeros(n)
    base = dict(mode=0, ind=(1, 16, 16), outd=(1, 16, 16), kd=1, sd=1, pd=0, cin=16, cout=64, in_stride=None, out_stride=None)
    ok = lambda **over: ops.winograd_supported(E.geom_of(base, **over))
    assert ok()
    assert not ok(cin=24), "Cin % 16"
    assert not ok(cin=8), "Cin % 16"
    assert ok(in_stride=20) and not ok(in_stride=18), "in_stride % 4"
    g = ops.geom(0, (1, 16, 16), (1, 8, 8), (1, 3, 3), (1, 2, 2), (0, 1, 1), 16, 64)
    assert not ops.winograd_supported(g), "stride 2"
    assert not ok(outd=(1, 16, 14)) and not ok(ind=(1, 18, 16)), "unequal maps"
    assert not ok(ind=(1, 1, 16), outd=(1, 1, 16)) and not ok(ind=(1, 16, 1), outd=(1, 16, 1)), "1 x N maps"
    assert ok(ind=(1, 2, 2), outd=(1, 2, 2))
    g = ops.geom(0, (1, 16, 16), (1, 16, 16), (1, 3, 3), (1, 1, 1), (0, 1, 1), 16, 256, ps=2, ps_channels=64)
    assert not ops.winograd_supported(g), "pixel shuffle"
    assert not ops.winograd_supported(E.geom_of(base), flags=ops.IN_RELU), "ReLU on load without a bnstate"
    # tail
    g64, g128 = E.geom_of(base, cin=64, mode=1), E.geom_of(base, cin=64, cout=128, mode=1)
    tail = (z(4096), z(4))
    sink_b = lambda c: ops.BnSink(c, 1, "cpu", dgamma=z(c), dbeta=z(c))
    sink_f = lambda c: ops.BnSink(c, 1, "cpu", gamma=z(c), beta=z(c), bnstate=z(4 * c))
    assert ops.winograd_supported(g64, tail=tail)
    assert not ops.winograd_supported(g128, tail=tail), "tail with Cout != 64"
    assert not ops.winograd_supported(E.geom_of(base, cin=64, mode=1, out_stride=96), tail=tail), "tail with out_stride != 64"
    assert not ops.winograd_supported(g64, tail=tail, flags=ops.ACCUMULATE), "tail with ACCUMULATE"
    assert not ops.winograd_supported(g64, tail=tail, flags=ops.OUT_RELU), "tail with OUT_RELU"
    assert not ops.winograd_supported(g64, tail=tail, bwd=(z(4), z(4), False)), "tail: bwd_y without a sink"
    # sinks
    bwd = (z(4), z(4), True)
    assert ops.winograd_supported(g64, bwd=bwd, sink=sink_b(64))
    assert not ops.winograd_supported(g64, bwd=bwd), "bwd_y without a backward sink"
    assert not ops.winograd_supported(g64, bwd=bwd, sink=sink_f(64)), "a forward sink with bwd_y"
    assert ops.winograd_supported(g64, sink=sink_f(64))
    # weight gradient
    wbase = dict(ind=(1, 16, 16), outd=(1, 16, 16), kd=1, sd=1, pd=0)
    wok = lambda **over: ops.wgrad_winograd_supported(E.geom_of(wbase, **over))
    assert wok()
    assert not wok(mode=1), "mode 1"
    assert not wok(cin=128) and not wok(cout=128), "128 channels"
    assert not wok(in_stride=80) and not wok(out_stride=80), "strided rows"
    assert not wok(ind=(1, 1, 16), outd=(1, 1, 16)), "1 x N maps"
    assert not wok(ind=(11, 16, 16), outd=(9, 16, 16), kd=3), "nine output planes"


def test_the_direct_form_serves_the_cross_checked_cases():
    """tests/test_gpu_wino_edges.py runs every case through ops.conv_forward too when lisec_conv_plan_query (answered on the
    host) accepts it: that is every case without a tail (the direct form carries a tail only in its two-line w-halo kernel,
    which these small maps do not take), so the cross-check cannot quietly shrink."""
    from lisec_amd import _lib, ops
    served = []
    for c in E.FWD:
        kw = extras_of(c)
        try:
            ops.conv_plan(E.geom_of(c), **kw)
            served.append(c["name"])
        except _lib.LisecError as e:
            print(f"{c['name']}: not served by the direct form: {e}")
    assert served == [c["name"] for c in E.FWD if not c["tail"]]
