"""CPU checks of the host side of predicted observations (no GPU): the entry points are exported and declared, the kind
constants agree between cugo_hip.h and Python, the null / negative-count paths answer CUGO_ERR_INVALID without a device,
and the Python methods exist.  Every test here fails before the feature exists."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest

cugo = importlib.import_module("cuda-bundle-adjustment_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_INVALID = -3


def header():
    with open(os.path.join(ROOT, "include", "cugo_hip.h")) as fh:
        return fh.read()


def test_entry_points_are_exported_and_declared():
    lib, h = cugo.lib(), header()
    for name in ("cugo_predict_observations", "cugo_graph_predict_observations"):
        assert hasattr(lib, name), name
        assert re.search(r"\bint %s\(" % name, h), name
    cpp = open(os.path.join(ROOT, "cuda-bundle-adjustment_amd", "include", "cuda_graph_optimisation.h")).read()
    assert re.search(r"\bbool predictObservations\(", cpp)
    # the calls that were there keep their declarations
    for name in ("cugo_reprojection_covariances", "cugo_graph_reprojection_covariances"):
        assert re.search(r"\bint %s\(" % name, h), name
    assert re.search(r"\bbool reprojectionCovariances\(", cpp)


def test_kind_constants_match_the_header():
    h = header()
    for name, value in (("MONO", 2), ("STEREO", 3), ("DEPTH", 4)):
        m = re.search(r"#define CUGO_OBS_%s (\d+)" % name, h)
        assert m and int(m.group(1)) == value == getattr(cugo, "OBS_" + name), name


def test_null_and_negative_counts_are_invalid_without_a_device():
    lib = cugo.lib()
    assert lib.cugo_predict_observations(None, 1, 1, *([None] * 13)) == ERR_INVALID
    assert b"cugo_predict_observations" in lib.cugo_last_error() and b"null" in lib.cugo_last_error()
    assert lib.cugo_predict_observations(None, 0, 0, *([None] * 13)) == ERR_INVALID      # (the context is required)
    assert lib.cugo_predict_observations(None, -1, 1, *([None] * 13)) == ERR_INVALID
    one = np.zeros(1, np.int32)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    out = np.zeros(9)
    f64 = out.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.cugo_graph_predict_observations(None, 1, i32(one), i32(one), 2, None, None, None, f64, f64) == ERR_INVALID
    assert b"cugo_graph_predict_observations" in lib.cugo_last_error()
    # a plan-only graph: refused before and after initialize(); null id lists and a negative count are invalid
    d = cugo.synth(6, 40, 160, seed=1)
    g = cugo.graph_from_arrays(d, plan_only=True)
    with pytest.raises(cugo.CugoError, match="error -3"):
        g.predict_observations([1], [2], cam=d["cam"])
    g.initialize()
    with pytest.raises(cugo.CugoError, match="plan-only"):
        g.predict_observations([1], [2], kind=cugo.OBS_STEREO, cam=d["cam"])
    assert lib.cugo_graph_predict_observations(g._g, 1, None, None, 2, None, None, None, f64, f64) == ERR_INVALID
    assert lib.cugo_graph_predict_observations(g._g, -1, i32(one), i32(one), 2, None, None, None, f64, f64) == ERR_INVALID
    g.close()


def test_python_methods_exist():
    assert callable(cugo.predict_observations)
    assert list(inspect.signature(cugo.predict_observations).parameters) == [
        "ctx", "n", "n_landmarks_free", "d_q_pose", "d_q_lm", "d_q_kind", "d_q_aa", "d_cam5", "d_cam_tab", "d_poses", "d_lms",
        "d_blocks", "d_cross18", "d_lmcov9", "d_z3", "d_cov9"]
    sig = inspect.signature(cugo.Graph.predict_observations)
    assert list(sig.parameters) == ["self", "pose_ids", "lm_ids", "kind", "cam", "sensor", "model"]
    assert sig.parameters["kind"].default == cugo.OBS_MONO == 2
    assert all(sig.parameters[k].default is None for k in ("cam", "sensor", "model"))
    with pytest.raises(ValueError):
        cugo.Graph.predict_observations(object(), [1, 2], [3])
