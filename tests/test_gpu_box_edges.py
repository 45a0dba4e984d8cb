"""lisec_rpn_labels and lisec_rpn_to_region (csrc/boxes.hip) through the C ABI, with a lisec_rpn_cfg of the test's own, on the
cases of tests/box_edge_cases.py against oracle/boxes_ref.py: small grids whose candidate counts are no multiple of the
workgroups, IoUs that are infinite, negative or exactly 0, bit-equal best IoUs (the fixup's first-in-loop-order rule), shared
and overwritten fixup anchors, 65 boxes, probability ties, a candidate list that runs out, and more than 256 picks.
Outputs start as NaN (labels: "all overwritten") or as a canary (NMS: the rows past out_count are not to be touched); the
workspace is exactly what lisec_*_workspace_bytes asks for, in front of canary bytes.  tests/test_box_edge_cases.py holds the
cases to the conditions that make these comparisons meaningful."""
import ctypes

import numpy as np
import pytest

import box_edge_cases as E

pytestmark = pytest.mark.gpu

EINVAL, ENOSPC = -1, -2                                        # LISEC_EINVAL, LISEC_ENOSPC
CANARY = 0x7ff8c0dec0dec0de                                    # a NaN with a payload: compared by its bits
BYTE = 0xA5
TAIL = 1024                                                    # canary bytes behind the workspace
PAD_ROWS = 8                                                   # canary rows behind out_boxes / out_probs


def _abi():
    import torch
    from lisec_amd import _lib
    return torch, _lib, _lib.load(), _lib.require_gpu()


def _rpn_cfg(cfg):
    from lisec_amd._lib import RpnCfg
    c = RpnCfg()
    c.outX, c.outY, c.vx, c.vy = cfg["outX"], cfg["outY"], cfg["vx"], cfg["vy"]
    for i, a in enumerate(cfg["anchors"]):
        for j in range(4):
            c.anchors[i][j] = float(a[j])
    return c


def _canaries(torch, dev, *shape):
    return torch.full(shape, CANARY, dtype=torch.int64, device=dev).view(torch.float64)


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def _arena(torch, dev, need):
    return torch.full((need + TAIL,), BYTE, dtype=torch.uint8, device=dev)


def _tail_intact(arena, need):
    return bool((arena[need:] == BYTE).all().item())


# ---- labels ----------------------------------------------------------------------------------------------------------------------
def _label_buffers(torch, dev, cfg):
    cells = cfg["outX"] * cfg["outY"]
    return [torch.full((cells * k,), float("nan"), dtype=torch.float64, device=dev) for k in (2, 2, 14)]


def _run_labels(c):
    torch, _lib, lib, dev = _abi()
    cfg, fixed = c["cfg"], c["fixed"]
    n = len(fixed)
    d_fixed = torch.from_numpy(np.array(fixed)).to(dev) if n else None
    valid, overlap, reg = _label_buffers(torch, dev, cfg)
    need = lib.lisec_rpn_labels_workspace_bytes(n)
    arena = _arena(torch, dev, need)
    _lib.check(lib.lisec_rpn_labels(ctypes.byref(_rpn_cfg(cfg)), _lib.ptr(d_fixed), n, E.IOU_LO, E.IOU_HI, _lib.ptr(arena), need,
                                    _lib.ptr(valid), _lib.ptr(overlap), _lib.ptr(reg), _lib.current_stream()))
    torch.cuda.synchronize()
    assert _tail_intact(arena, need), "lisec_rpn_labels wrote behind the workspace it asked for"
    shape = (cfg["outX"], cfg["outY"])
    return valid.cpu().numpy().reshape(*shape, 2), overlap.cpu().numpy().reshape(*shape, 2), reg.cpu().numpy().reshape(*shape, 14)


@pytest.mark.parametrize("name", list(E.LABEL_CASES))
def test_labels_vs_oracle(name):
    c = E.label_case(name)
    valid, overlap, reg = _run_labels(c)
    for what, a in (("valid", valid), ("overlap", overlap), ("out_regress", reg)):
        assert not np.isnan(a).any(), f"{what}: {int(np.isnan(a).sum())} elements never written"
    assert np.array_equal(valid, c["valid"]), f"valid differs at {np.argwhere(valid != c['valid'])[:4].tolist()}"
    assert np.array_equal(overlap, c["overlap"]), f"overlap differs at {np.argwhere(overlap != c['overlap'])[:4].tolist()}"
    got = reg + np.repeat(overlap, 7, axis=2)                  # what preprocessLabels returns (serialize_data.py:338)
    err = np.abs(got - c["reg"])
    print(f"{name}: max |out_regress - oracle| = {err.max():.3e}")
    assert np.allclose(got, c["reg"], rtol=1e-12, atol=1e-12)
    if c["cfg"]["exact"]:
        # differences and IEEE quotients of dyadic numbers, and log(1): x, y, z, yaw and every log term that is 0
        exact = np.zeros(14, dtype=bool)
        exact[[0, 1, 2, 6, 7, 8, 9, 13]] = True
        exact = exact[None, None, :] | (c["reg"] == np.repeat(c["overlap"], 7, axis=2))
        assert np.array_equal(got[exact], c["reg"][exact])
    again = _run_labels(c)
    for a, b in zip((valid, overlap, reg), again):
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), "two runs differ"


def test_labels_refusals():
    torch, _lib, lib, dev = _abi()
    c = E.label_case("fixup_tie")
    cfg, n = c["cfg"], len(c["fixed"])
    d_fixed = torch.from_numpy(np.array(c["fixed"])).to(dev)
    cells = cfg["outX"] * cfg["outY"]
    outs = [_canaries(torch, dev, cells * k) for k in (2, 2, 14)]
    need = lib.lisec_rpn_labels_workspace_bytes(n)
    arena = _arena(torch, dev, need)
    good, odd = _rpn_cfg(cfg), _rpn_cfg(dict(cfg, outX=cfg["outX"] - 1))

    def call(rpn=good, boxes=d_fixed, ws=arena, ws_bytes=need, o=outs):
        return lib.lisec_rpn_labels(ctypes.byref(rpn), _lib.ptr(boxes), n, E.IOU_LO, E.IOU_HI, _lib.ptr(ws), ws_bytes,
                                    _lib.ptr(o[0]), _lib.ptr(o[1]), _lib.ptr(o[2]), _lib.current_stream())

    assert call(ws_bytes=need - 1) == ENOSPC
    assert call(rpn=odd) == EINVAL
    assert call(ws=None) == EINVAL
    assert call(boxes=None) == EINVAL
    for k in range(3):
        assert call(o=[None if i == k else t for i, t in enumerate(outs)]) == EINVAL
    torch.cuda.synchronize()
    assert all((_bits(t) == np.int64(CANARY)).all() for t in outs), "a refused call wrote to an output"
    assert bool((arena == BYTE).all().item()), "a refused call wrote to the workspace"


# ---- decode + NMS ----------------------------------------------------------------------------------------------------------------
def _head_views(torch, dev, c, strided):
    """(cls, cls_stride, reg, reg_stride) on the device: dense maps, or the two column ranges of one (M, 16) head buffer."""
    cls = torch.from_numpy(np.array(c["cls"])).to(dev).reshape(-1, 2)
    reg = torch.from_numpy(np.array(c["reg"])).to(dev).reshape(-1, 14)
    if not strided:
        return cls, 2, reg, 14
    head = torch.cat([cls, reg], 1).contiguous()
    return head[:, :2], head.stride(0), head[:, 2:], head.stride(0)


def _run_nms(c, strided):
    torch, _lib, lib, dev = _abi()
    rpn = _rpn_cfg(c["cfg"])
    cls, cls_stride, reg, reg_stride = _head_views(torch, dev, c, strided)
    rows = c["max_boxes"] + 1
    out_boxes, out_probs = _canaries(torch, dev, rows + PAD_ROWS, 7), _canaries(torch, dev, rows + PAD_ROWS)
    count = torch.full((1,), -777, dtype=torch.int32, device=dev)
    need = lib.lisec_rpn_to_region_workspace_bytes(ctypes.byref(rpn), c["max_boxes"])
    arena = _arena(torch, dev, need)
    _lib.check(lib.lisec_rpn_to_region(ctypes.byref(rpn), _lib.ptr(cls), cls_stride, _lib.ptr(reg), reg_stride, float(c["thresh"]),
                                       c["max_boxes"], _lib.ptr(arena), need, _lib.ptr(out_boxes), _lib.ptr(out_probs),
                                       _lib.ptr(count), _lib.current_stream()))
    torch.cuda.synchronize()
    assert _tail_intact(arena, need), "lisec_rpn_to_region wrote behind the workspace it asked for"
    return int(count.item()), out_boxes.cpu().numpy(), out_probs.cpu().numpy()


@pytest.mark.parametrize("name", list(E.NMS_CASES))
def test_rpn_to_region_vs_oracle(name):
    c = E.nms_case(name)
    picks = c["picks"]
    k, boxes, probs = _run_nms(c, strided=False)
    print(f"{name}: out_count {k}, oracle {len(picks)} picks")
    assert k == len(picks)
    unwritten = np.flatnonzero(probs[:k].view(np.int64) == np.int64(CANARY))
    assert not len(unwritten), f"rows {unwritten[0]} .. {unwritten[-1]} of {k} reported picks were never written"
    assert np.array_equal(probs[:k], c["probs"][picks])
    err = np.abs(boxes[:k] - c["boxes"][picks])
    print(f"{name}: max |out_boxes - oracle| = {err.max():.3e}")
    assert np.allclose(boxes[:k], c["boxes"][picks], rtol=1e-12, atol=1e-12)
    assert (boxes[k:].view(np.int64) == np.int64(CANARY)).all() and (probs[k:].view(np.int64) == np.int64(CANARY)).all(), \
        "a row at or past out_count was written"
    # the (M, 16) head view (strides 16 / 16), and a second dense run: equal bits
    for strided in (True, False):
        k2, boxes2, probs2 = _run_nms(c, strided=strided)
        assert k2 == k and np.array_equal(boxes2.view(np.int64), boxes.view(np.int64)) and \
            np.array_equal(probs2.view(np.int64), probs.view(np.int64)), f"strided={strided}: another run differs"


def test_rpn_to_region_refusals():
    torch, _lib, lib, dev = _abi()
    c = E.nms_case("exhausted")
    cfg, max_boxes = c["cfg"], c["max_boxes"]
    good, odd = _rpn_cfg(cfg), _rpn_cfg(dict(cfg, outX=cfg["outX"] - 1))
    cls, _, reg, _ = _head_views(torch, dev, c, strided=False)
    rows = max_boxes + 1
    outs = dict(boxes=_canaries(torch, dev, rows, 7), probs=_canaries(torch, dev, rows),
                count=torch.full((2,), CANARY, dtype=torch.int64, device=dev))
    need = lib.lisec_rpn_to_region_workspace_bytes(ctypes.byref(good), max_boxes)
    assert need > 0 and lib.lisec_rpn_to_region_workspace_bytes(ctypes.byref(good), -1) == 0
    assert lib.lisec_rpn_to_region_workspace_bytes(ctypes.byref(odd), max_boxes) == 0
    arena = _arena(torch, dev, need)

    def call(rpn=good, cls_stride=2, reg_stride=14, cap=max_boxes, ws=arena, ws_bytes=need, **null):
        o = {k: None if k in null else t for k, t in outs.items()}
        return lib.lisec_rpn_to_region(ctypes.byref(rpn), _lib.ptr(cls), cls_stride, _lib.ptr(reg), reg_stride, float(c["thresh"]),
                                       cap, _lib.ptr(ws), ws_bytes, _lib.ptr(o["boxes"]), _lib.ptr(o["probs"]), _lib.ptr(o["count"]),
                                       _lib.current_stream())

    assert call(ws_bytes=need - 1) == ENOSPC
    assert call(rpn=odd) == EINVAL
    assert call(cls_stride=1) == EINVAL
    assert call(reg_stride=13) == EINVAL
    assert call(cap=-1) == EINVAL
    assert call(ws=None) == EINVAL
    for k in outs:
        assert call(**{k: True}) == EINVAL
    torch.cuda.synchronize()
    assert all((_bits(t) == np.int64(CANARY)).all() for t in outs.values()), "a refused call wrote to an output"
    assert bool((arena == BYTE).all().item()), "a refused call wrote to the workspace"
