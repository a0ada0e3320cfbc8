"""CPU: tests/dataset_restate.py (the numpy statement of DynDataset.__getitem__ as a function of (sample, draws)) against the
five fixtures recorded from the reference, and the host-side argument errors of DeviceDynDataset."""
import copy

import numpy as np
import pytest

import dataset_restate as DR

CASES = ["dataset_rope", "dataset_cloth", "dataset_granular", "dataset_backoff", "dataset_softbody"]
TENSORS = ["state", "action", "eef_future", "action_future", "state_future"]


@pytest.fixture(scope="module", params=CASES)
def case(request):
    fx = DR.load_fixture(request.param)
    got = DR.restate_batch(*DR.dataset_args(fx), fx["samples"], fx["draws"])
    return request.param, fx, got


def test_fixture_contents():
    """What the issue's table promises of each case."""
    fx = DR.load_fixture("dataset_rope")
    assert sorted(o.shape[1] for o in fx["obj_pos"]) == [37, 600, 601] and fx["draws"]["rot"] is not None and len(fx["samples"]) == 6
    assert fx["eef_pos"][0].shape[1] == 1
    steps = [len(t) - 1 for t in DR.load_fixture("dataset_backoff")["trail"]]
    assert sum(s >= 1 for s in steps) >= 2 and sum(s == 0 for s in steps) >= 1
    fx = DR.load_fixture("dataset_softbody")
    d = fx["dataset_config"]
    assert d["n_his"] == 5 and d["store_rest_state"] and fx["pair_lists"].shape[1] - 1 == d["n_his"] - 1 + d["n_future"]
    assert d["datasets"][0]["connect_tool_all_non_fixed"] and d["datasets"][0]["min_knn"] < 1.0
    assert DR.load_fixture("dataset_cloth")["eef_pos"][0].shape[1] == 2 and DR.load_fixture("dataset_granular")["eef_pos"][0].shape[1] == 5


def test_indices_masks_and_edges_are_equal(case):
    name, fx, got = case
    want = fx["want"]
    for k in ("attrs", "p_rigid", "p_instance", "obj_mask", "material_index"):
        assert np.array_equal(got[k], want[k]), (name, k)
        assert got[k].dtype == want[k].dtype, (name, k, got[k].dtype, want[k].dtype)
    assert np.array_equal(got["physics_param"], want[fx["material"] + "_physics_param"])
    for b in range(len(fx["samples"])):
        assert len(got["fps_idx"][b]) == int(want["obj_mask"][b].sum())
        assert np.array_equal(got["recv"][b], want["recv"][b]) and np.array_equal(got["send"][b], want["send"][b]), (name, b)
        assert [tuple(r) for r in got["trail"][b]] == fx["trail"][b], (name, b)


def test_tensors(case):
    """Un-augmented fixtures are bit-equal; the augmented one (rope) is within the rotation bound, its z bit-equal."""
    name, fx, got = case
    want = fx["want"]
    for k in TENSORS:
        assert got[k].shape == want[k].shape and got[k].dtype == np.float32
        if fx["draws"]["rot"] is None:
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (name, k)
        else:
            assert np.array_equal(got[k][..., 2], want[k][..., 2]), (name, k)
            err = np.abs(got[k][..., :2].astype(np.float64) - want[k][..., :2])
            assert (err <= DR.rotation_bound(want[k])).all(), (name, k, float(err.max()))


def test_stage2_is_the_references_fps_rad_idx_on_ties_and_extremes():
    """fps_stage2 on duplicates (all distances equal: the lowest index wins), radius 0 and a radius above the cloud."""
    rng = np.random.default_rng(0)
    p = rng.normal(size=(50, 3)).astype(np.float32)
    assert DR.fps_stage2(p, 100.0, 7).tolist() == [7]
    assert sorted(DR.fps_stage2(p, 0.0, 3).tolist()) == list(range(50))
    dup = np.repeat(p[:1], 9, 0)
    assert DR.fps_stage1(dup, 9, 4).tolist() == [4] + [0] * 8
    assert DR.fps_stage2(dup, 0.0, 2).tolist() == [2]
    two = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [-1, 0, 0]], np.float32)
    assert DR.fps_stage1(two, 3, 0).tolist() == [0, 1, 3]


# ---- host-side argument errors: raised before the device is touched, so they need no GPU
def _args(name="dataset_cloth"):
    fx = DR.load_fixture(name)
    return [copy.deepcopy(a) for a in DR.dataset_args(fx)]


def test_a_cloud_above_the_limit_is_refused_on_the_host():
    from adaptigraph_amd.dataset import DeviceDynDataset, FPS_MAX_POINTS
    a = _args()
    T = a[4][0].shape[0]
    a[4][0] = np.zeros((T, FPS_MAX_POINTS + 1, 3), np.float32)
    with pytest.raises(NotImplementedError, match=str(FPS_MAX_POINTS)):
        DeviceDynDataset(*a, device="cpu")


def test_pair_length_is_checked_against_n_his_and_n_future():
    from adaptigraph_amd.dataset import DeviceDynDataset
    a = _args()
    a[2] = a[2][:, :-1]                                     # 6 frames, no rest state: n_his + n_future = 7
    with pytest.raises(AssertionError, match="n_his"):
        DeviceDynDataset(*a, device="cpu")
    a = _args("dataset_softbody")                           # 7 frames + the rest state = 8: fine; 6 is not
    a[2] = a[2][:, :-1]
    with pytest.raises(AssertionError, match="rest state"):
        DeviceDynDataset(*a, device="cpu")


def test_more_than_one_dataset_or_material_is_refused():
    from adaptigraph_amd.dataset import DeviceDynDataset
    a = _args()
    a[0]["datasets"] = a[0]["datasets"] * 2
    with pytest.raises(AssertionError, match="Only one object type"):
        DeviceDynDataset(*a, device="cpu")
    a = _args()
    a[0]["materials"] = ["cloth", "rope"]
    with pytest.raises(AssertionError, match="single material"):
        DeviceDynDataset(*a, device="cpu")


def test_valid_arguments_reach_the_device_check():
    """With valid arguments the constructor gets as far as asking for a GPU (no CPU fallback)."""
    from adaptigraph_amd.dataset import DeviceDynDataset
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceDynDataset(*_args(), device="cpu")


def test_ctypes_batch_struct_matches_the_header(tmp_path):
    """AgDatasetBatch (adaptigraph_amd/_lib.py) against ag_dataset_batch as a C compiler lays it out: size and every field's offset."""
    import os
    import subprocess
    from adaptigraph_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [n for n, _ in _lib.AgDatasetBatch._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "adaptigraph_amd.h"\nint main(void) {\n'
    src += '  printf("%zu\\n", sizeof(ag_dataset_batch));\n'
    src += "".join(f'  printf("%zu\\n", offsetof(ag_dataset_batch, {n}));\n' for n in names) + "  return 0;\n}\n"
    (tmp_path / "t.c").write_text(src)
    exe = str(tmp_path / "t")
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(tmp_path / "t.c"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    import ctypes
    assert got == [ctypes.sizeof(_lib.AgDatasetBatch)] + [getattr(_lib.AgDatasetBatch, n).offset for n in names]
