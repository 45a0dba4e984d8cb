"""lisec_amd.regularizers (tf.keras.regularizers of 2.4), the chunk table of the penalty pass and the regularizers in a
Keras .h5 -- everything about the weight regularizers that needs no GPU."""
import inspect
import json
import math
import struct
import types

import numpy as np
import pytest

from lisec_amd import _lib, keras_h5, ops, regularizers
from lisec_amd.params import TRAINABLE_KINDS, glorot_numpy, param_specs


def f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_classes_and_shorthands():
    assert regularizers.l1 is regularizers.L1 and regularizers.l2 is regularizers.L2
    assert regularizers.L1L2().get_config() == {"l1": 0.0, "l2": 0.0}
    assert regularizers.L1().get_config() == {"l1": f32(0.01)}
    assert regularizers.L2().get_config() == {"l2": f32(0.01)}
    r = regularizers.l1_l2(l1=0.5, l2=0.25)
    assert type(r) is regularizers.L1L2 and r.pair() == (0.5, 0.25)
    assert regularizers.l1_l2().pair() == (f32(0.01), f32(0.01))
    assert regularizers.L2(l=0.5).pair() == (0.0, 0.5) and regularizers.L1(l=0.5).pair() == (0.5, 0.0)


def test_coefficients_are_float32_rounded_python_floats():
    r = regularizers.l2(1e-4)
    assert isinstance(r.l2, float) and r.l2 == f32(1e-4) and r.l2 != 1e-4
    assert regularizers.serialize(r) == {"class_name": "L2", "config": {"l2": f32(1e-4)}}
    r = regularizers.L1L2(l1=0.1, l2=1e-3)
    assert r.get_config() == {"l1": f32(0.1), "l2": f32(1e-3)}
    assert all(isinstance(v, float) for v in r.get_config().values())
    assert regularizers.L1(np.float64(0.3)).l1 == f32(0.3)


def test_get_serialize_deserialize_round_trips():
    assert regularizers.get(None) is None and regularizers.serialize(None) is None
    r = regularizers.l2(1e-4)
    assert regularizers.get(r) is r
    assert type(regularizers.get("l1")) is regularizers.L1 and regularizers.get("l1").pair() == (f32(0.01), 0.0)
    assert type(regularizers.get("l2")) is regularizers.L2 and regularizers.get("l2").pair() == (0.0, f32(0.01))
    assert type(regularizers.get("l1_l2")) is regularizers.L1L2
    assert regularizers.get("l1_l2").pair() == (f32(0.01), f32(0.01))
    for reg in (regularizers.L1(0.3), regularizers.L2(1e-4), regularizers.L1L2(0.2, 0.7), regularizers.L1L2()):
        ser = regularizers.serialize(reg)
        assert set(ser) == {"class_name", "config"} and ser["class_name"] == type(reg).__name__
        assert json.loads(json.dumps(ser)) == ser
        for back in (regularizers.deserialize(ser), regularizers.get(ser)):
            assert type(back) is type(reg) and back.pair() == reg.pair()
            assert regularizers.serialize(back) == ser
    assert regularizers.serialize("l2") == {"class_name": "L2", "config": {"l2": f32(0.01)}}


@pytest.mark.parametrize("bad", [-1e-4, float("nan"), float("inf"), -float("inf"), 1e39])
def test_bad_coefficients_raise_value_error(bad):
    for make in (lambda: regularizers.L1(bad), lambda: regularizers.L2(bad), lambda: regularizers.L1L2(l1=bad),
                 lambda: regularizers.L1L2(l2=bad), lambda: regularizers.l1_l2(bad, 0.1),
                 lambda: regularizers.get({"class_name": "L2", "config": {"l2": bad}})):
        with pytest.raises(ValueError):
            make()


def test_unknown_names_raise_value_error():
    for bad in ("l3", "L1L3", {"class_name": "Orthogonal", "config": {}}, {"config": {}}, 3):
        with pytest.raises(ValueError):
            regularizers.get(bad)


def test_a_regularizer_of_ones_own_is_refused():
    class Mine(regularizers.Regularizer):
        def __call__(self, x):
            return 0.0

    class Twisted(regularizers.L2):
        def __call__(self, x):
            return 1.0

    for own in (lambda w: 0.0, Mine(), Twisted(0.1)):
        with pytest.raises(NotImplementedError, match="of one's own"):
            regularizers.get(own)
    with pytest.raises(NotImplementedError):
        regularizers.L2(0.1)(np.zeros(3))
    with pytest.raises(NotImplementedError):
        regularizers.deserialize({"class_name": "Mine", "config": {}}, custom_objects={"Mine": Mine})

    class Renamed(regularizers.L2):              # no arithmetic of its own: the kernels compute it
        pass
    assert regularizers.get(Renamed(0.5)).pair() == (0.0, 0.5)
    # ... and it is written under the built-in name, which deserialize knows
    ser = regularizers.serialize(Renamed(0.5))
    assert ser == {"class_name": "L2", "config": {"l2": 0.5}}
    assert type(regularizers.deserialize(ser)) is regularizers.L2 and regularizers.get(ser).pair() == (0.0, 0.5)


def test_coefficients_by_kind_over_param_specs():
    specs = param_specs()
    c = regularizers.coefficients(specs, kernel=regularizers.l2(1e-4), gamma="l1")
    kinds = {n: k for n, _, k in specs}
    assert set(c) == {n for n, k in kinds.items() if k in ("kernel", "gamma")}
    assert all(c[n] == ((0.0, f32(1e-4)) if kinds[n] == "kernel" else (f32(0.01), 0.0)) for n in c)
    assert regularizers.coefficients(specs) == {}
    assert regularizers.coefficients(specs, kernel=regularizers.L1L2(), bias=regularizers.L2(0.0)) == {}
    assert list(c) == [n for n, _, k in specs if k in ("kernel", "gamma")]          # forward order


def test_create_model_signature():
    from lisec_amd import model_training as mt
    assert mt.regularizers is regularizers
    for fn, first in ((mt.createModel, 0), (mt.Model.__init__, 1)):
        params = inspect.signature(fn).parameters
        names = list(params)
        assert names[first:first + 4] == ["nx", "ny", "nz", "maxPoints"]
        for kw in ("kernel_regularizer", "bias_regularizer", "gamma_regularizer", "beta_regularizer",
                   "activity_regularizer"):
            assert params[kw].default is None
    assert list(inspect.signature(mt.Model.__init__).parameters)[5] == "params"      # positional use as before
    with pytest.raises(NotImplementedError, match="activity_regularizer"):
        mt.createModel(16, 32, 8, 35, activity_regularizer=regularizers.l2(0.1))
    with pytest.raises(NotImplementedError, match="of one's own"):
        mt.createModel(16, 32, 8, 35, kernel_regularizer=lambda w: 0.0)
    with pytest.raises(ValueError):
        mt.createModel(16, 32, 8, 35, bias_regularizer=regularizers_l2_negative())


def regularizers_l2_negative():
    return {"class_name": "L2", "config": {"l2": -1.0}}


# ---- the chunk table ------------------------------------------------------------------------------------------------
def _layout(dprime=1):
    """ParamStore's layout of theta, restated: every trainable variable at a multiple of 4 floats, in spec order."""
    offsets, nt = {}, 0
    for name, shape, kind in param_specs(dprime):
        n = int(np.prod(shape))
        if kind in TRAINABLE_KINDS:
            offsets[name] = ("theta", nt, shape)
            nt += (n + 3) // 4 * 4
        else:
            offsets[name] = ("state", 0, shape)
    return types.SimpleNamespace(offsets=offsets, n_theta=nt)


def test_layout_restatement_is_param_stores():
    import torch
    from lisec_amd.params import ParamStore
    store, lay = ParamStore(torch.device("cpu")), _layout()
    assert lay.n_theta == store.n_theta
    assert all(store.offsets[n][:2] == lay.offsets[n][:2] for n in store.trainable_names())


@pytest.mark.parametrize("which", ["kernels", "mixed", "all"])
def test_reg_chunks_on_the_real_specs(which):
    lay, specs = _layout(), param_specs()
    if which == "kernels":
        coeffs = regularizers.coefficients(specs, kernel=regularizers.l2(1e-4))
    elif which == "all":
        coeffs = regularizers.coefficients(specs, kernel="l2", bias="l1", gamma="l1_l2", beta=regularizers.l1(0.5))
    else:
        coeffs = {"cls.bias": (0.5, 0.0), "vfe1.dense.kernel": (0.0, 0.25), "rpn2.conv3.kernel": (0.125, 0.5),
                  "mid2.bn.gamma": (0.0, 0.0), "up3.kernel": (1.0, 0.0)}
    rows = ops.reg_chunks(lay, coeffs)
    assert _lib.REG_CHUNK == 4096
    offs = [r[0] for r in rows]
    assert offs == sorted(offs) and len(set(offs)) == len(offs)                      # ascending
    spans = {n: (o, o + (int(np.prod(s)) + 3) // 4 * 4) for n, (w, o, s) in lay.offsets.items() if w == "theta"}
    live = {n for n, p in coeffs.items() if p != (0.0, 0.0)}
    covered = {n: [] for n in live}
    for off, count, l1, l2, flags in rows:
        assert flags == 0                                                            # no variable named as unwritten
        assert off % 4 == 0 and count % 4 == 0 and 0 < count <= _lib.REG_CHUNK
        owner = [n for n, (a, b) in spans.items() if a <= off < b]
        assert len(owner) == 1 and owner[0] in live, "a chunk of an unregularised variable"
        a, b = spans[owner[0]]
        assert off + count <= b, "a chunk crosses a variable"
        assert (l1, l2) == coeffs[owner[0]]
        covered[owner[0]].append((off, count))
    for n in live:                                                                   # exactly once, up to the padded length
        a, b = spans[n]
        pos = a
        for off, count in covered[n]:
            assert off == pos
            pos += count
        assert pos == b and len(covered[n]) == math.ceil((b - a) / _lib.REG_CHUNK)
    assert rows[-1][0] + rows[-1][1] <= lay.n_theta


def test_reg_chunks_refusals_and_empty():
    lay = _layout()
    assert ops.reg_chunks(lay, {}) == [] and ops.reg_chunks(lay, {"cls.kernel": (0.0, 0.0)}) == []
    with pytest.raises(KeyError):
        ops.reg_chunks(lay, {"no.such.kernel": (0.1, 0.0)})
    with pytest.raises(ValueError):
        ops.reg_chunks(lay, {"mid1.bn.moving_mean": (0.1, 0.0)})


def test_reg_chunks_flag_the_variables_no_backward_writes():
    """The chunks of a variable named in `unwritten` carry REG_GRAD_IS_ZERO (the pass stores its term there); no other."""
    lay = _layout()
    coeffs = regularizers.coefficients(param_specs(), bias=regularizers.l1_l2(0.5, 0.25), kernel="l2")
    unwritten = ["mid2.conv.bias", "rpn3.conv4.bias", "rpn1.conv0.kernel", "mid1.bn.gamma"]     # the last: not in coeffs
    rows = ops.reg_chunks(lay, coeffs, unwritten=unwritten)
    assert [r[:4] for r in rows] == [r[:4] for r in ops.reg_chunks(lay, coeffs)]
    flagged = {n for n in coeffs for r in rows
               if r[4] and lay.offsets[n][1] <= r[0] < lay.offsets[n][1] + int(np.prod(lay.offsets[n][2]))}
    assert flagged == set(unwritten[:3]) and {r[4] for r in rows} == {0, _lib.REG_GRAD_IS_ZERO}
    assert sum(r[4] for r in rows) == 1 + 1 + math.ceil(9 * 64 * 128 / _lib.REG_CHUNK)


def test_reg_chunk_record_matches_the_header():
    import ctypes
    import os
    import re
    assert ctypes.sizeof(_lib.RegChunk) == 24 and _lib.RegChunk.offset.offset == 0 and _lib.RegChunk.count.offset == 8
    assert _lib.RegChunk.l1.offset == 12 and _lib.RegChunk.l2.offset == 16 and _lib.RegChunk.flags.offset == 20
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lisec_hip.h")).read()
    assert int(re.search(r"#define LISEC_REG_GRAD_IS_ZERO (\d+)", header).group(1)) == _lib.REG_GRAD_IS_ZERO == 1
    assert int(re.search(r"#define LISEC_REG_CHUNK (\d+)", header).group(1)) == _lib.REG_CHUNK
    assert "lisec_regularize(" in header and "lisec_regularize_workspace_bytes(" in header


# ---- the Keras file -------------------------------------------------------------------------------------------------
GRID = (16, 32, 8, 35)


def _read_config(path):
    from lisec_amd import hdf5_lite
    with hdf5_lite.File(path, "r") as f:
        v = f.attrs["model_config"]
    return json.loads(bytes(v).decode("utf8") if isinstance(v, (bytes, np.bytes_)) else str(v))


def _rewrite_config(src, dst, edit):
    """Copies the Keras file src to dst with model_config passed through edit(cfg)."""
    from lisec_amd import hdf5_lite
    cfg = _read_config(src)
    edit(cfg)
    ck = keras_h5.load_model(src)
    keras_h5.save_model(dst, ck["params"], *GRID)
    with hdf5_lite.File(dst, "r") as f:
        names = [bytes(x).decode() for x in np.asarray(f["model_weights"].attrs["layer_names"]).ravel()]
        weights = {n: {bytes(w).decode(): f["model_weights"][n][bytes(w).decode()][()]
                       for w in np.asarray(f["model_weights"][n].attrs["weight_names"]).ravel()} for n in names}
    with hdf5_lite.File(dst, "w") as f:
        f.attrs["keras_version"] = keras_h5.KERAS_VERSION.encode()
        f.attrs["backend"] = b"tensorflow"
        f.attrs["model_config"] = json.dumps(cfg).encode("utf8")
        g = f.create_group("model_weights")
        g.attrs["layer_names"] = [n.encode() for n in names]
        for n in names:
            lg = g.create_group(n)
            lg.attrs["weight_names"] = [w.encode() for w in weights[n]]
            for w, a in weights[n].items():
                lg.create_dataset(w, data=a)


def test_h5_uniform_l2_on_kernels_round_trips(tmp_path):
    params = glorot_numpy(seed=3)
    coeffs = regularizers.coefficients(param_specs(), kernel=regularizers.l2(1e-4))
    path = str(tmp_path / "l2.h5")
    keras_h5.save_model(path, params, *GRID, regularizers=coeffs)
    ck = keras_h5.load_model(path)
    assert ck["regularizers"] == coeffs
    for name in params:
        np.testing.assert_array_equal(ck["params"][name], params[name])
    layers = _read_config(path)["config"]["layers"]
    want = {"class_name": "L2", "config": {"l2": f32(1e-4)}}
    seen = 0
    for L in layers:
        c = L["config"]
        if L["class_name"] in ("Dense", "Conv3D", "Conv2D", "Conv2DTranspose"):
            assert c["kernel_regularizer"] == want and "bias_regularizer" not in c
            seen += 1
        else:
            assert not any(k.endswith("_regularizer") for k in c)
    assert seen == sum(k == "kernel" for _, _, k in param_specs())


def test_h5_all_four_kinds_round_trip(tmp_path):
    coeffs = regularizers.coefficients(param_specs(), kernel=regularizers.l1_l2(0.5, 0.25), bias=regularizers.l1(0.125),
                                       gamma=regularizers.l2(2.0), beta="l1")
    path = str(tmp_path / "four.h5")
    keras_h5.save_model(path, glorot_numpy(seed=3), *GRID, regularizers=coeffs)
    assert keras_h5.load_model(path)["regularizers"] == coeffs
    bn = next(L for L in _read_config(path)["config"]["layers"] if L["class_name"] == "BatchNormalization")
    assert bn["config"]["gamma_regularizer"] == {"class_name": "L2", "config": {"l2": 2.0}}
    assert bn["config"]["beta_regularizer"] == {"class_name": "L1", "config": {"l1": f32(0.01)}}


def test_h5_mixed_per_layer_set_built_by_editing_the_json(tmp_path):
    """Different regularizers on different layers, null where Keras writes null: what a file of Keras' own may hold."""
    src, dst = str(tmp_path / "plain.h5"), str(tmp_path / "mixed.h5")
    keras_h5.save_model(src, glorot_numpy(seed=3), *GRID)
    layers, _ = keras_h5.keras_layers(*GRID)
    by_name = {L["name"]: dict(L["weights"]) for L in layers}

    def edit(cfg):
        for L in cfg["config"]["layers"]:
            c = L["config"]
            if L["class_name"] in ("Dense", "Conv3D", "Conv2D", "Conv2DTranspose"):
                c.update(kernel_regularizer=None, bias_regularizer=None, activity_regularizer=None)
            if L["name"] == "conv3d_1":
                c["kernel_regularizer"] = {"class_name": "L2", "config": {"l2": 0.5}}
                c["bias_regularizer"] = {"class_name": "L1", "config": {"l1": 0.25}}
            if L["name"] == "dense":
                c["kernel_regularizer"] = {"class_name": "L1L2", "config": {"l1": 0.125, "l2": 2.0}}
                c["bias_regularizer"] = {"class_name": "L2", "config": {"l2": 1.0}}     # use_bias=False: no variable
            if L["name"] == "batch_normalization_4":
                c["beta_regularizer"] = {"class_name": "L1", "config": {"l1": 4.0}}
                c["gamma_regularizer"] = {"class_name": "L1L2", "config": {"l1": 0.0, "l2": 0.0}}
            if L["name"] == "ClassificationLayer":
                c["bias_regularizer"] = {"class_name": "L2", "config": {"l2": 8.0}}

    _rewrite_config(src, dst, edit)
    got = keras_h5.load_model(dst)["regularizers"]
    assert got == {by_name["conv3d_1"]["kernel"]: (0.0, 0.5), by_name["conv3d_1"]["bias"]: (0.25, 0.0),
                   by_name["dense"]["kernel"]: (0.125, 2.0), by_name["batch_normalization_4"]["beta"]: (4.0, 0.0),
                   "cls.bias": (0.0, 8.0)}
    # ... and written again, the same per-variable set comes back
    again = str(tmp_path / "again.h5")
    keras_h5.save_model(again, glorot_numpy(seed=3), *GRID, regularizers=got)
    assert keras_h5.load_model(again)["regularizers"] == got


def test_h5_without_regularizers_keeps_its_bytes(tmp_path):
    params = glorot_numpy(seed=3)
    opt = dict(lr=0.01, decay=1e-6, momentum=0.9, nesterov=True)
    paths = [str(tmp_path / f"{i}.h5") for i in range(4)]
    keras_h5.save_model(paths[0], params, *GRID, optimizer=opt)
    keras_h5.save_model(paths[1], params, *GRID, optimizer=opt, regularizers=None)
    keras_h5.save_model(paths[2], params, *GRID, optimizer=opt, regularizers={})
    keras_h5.save_model(paths[3], params, *GRID, optimizer=opt, regularizers={"cls.kernel": (0.0, 0.0)})
    blobs = [open(p, "rb").read() for p in paths]
    assert blobs[0] == blobs[1] == blobs[2] == blobs[3]
    assert b"_regularizer" not in blobs[0]
    assert keras_h5.load_model(paths[0])["regularizers"] == {}
    assert keras_h5.model_config(*GRID) == keras_h5.model_config(*GRID, regularizers=None)


def test_h5_refusals_name_the_layer(tmp_path):
    src = str(tmp_path / "plain.h5")
    keras_h5.save_model(src, glorot_numpy(seed=3), *GRID)

    def activity(cfg):
        L = next(L for L in cfg["config"]["layers"] if L["name"] == "conv2d_3")
        L["config"]["activity_regularizer"] = {"class_name": "L2", "config": {"l2": 0.5}}

    def unknown(cfg):
        L = next(L for L in cfg["config"]["layers"] if L["name"] == "conv2d_transpose_1")
        L["config"]["kernel_regularizer"] = {"class_name": "OrthogonalRegularizer", "config": {"factor": 0.01}}

    for edit, layer in ((activity, "conv2d_3"), (unknown, "conv2d_transpose_1")):
        dst = str(tmp_path / f"{layer}.h5")
        _rewrite_config(src, dst, edit)
        with pytest.raises(NotImplementedError, match=layer):
            keras_h5.load_model(dst)
    with pytest.raises(KeyError):
        keras_h5.model_config(*GRID, regularizers={"no.such.kernel": (0.0, 0.5)})
    with pytest.raises(ValueError, match="moving_mean"):         # not silently dropped: ops.reg_chunks refuses it too
        keras_h5.model_config(*GRID, regularizers={"mid1.bn.moving_mean": (0.0, 0.5)})
    with pytest.raises(ValueError):
        keras_h5.save_model(str(tmp_path / "bad.h5"), glorot_numpy(seed=3), *GRID,
                            regularizers={"rpn1.bn0.moving_variance": (0.5, 0.0)})
