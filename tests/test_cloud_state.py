"""CPU checks of adaptigraph_amd.perception (-m "not gpu"): the declaration of ag_fps_cloud, the argument errors that come from
the host, the order in which numpy's generator is consumed, and the padded layout against a numpy restatement of the reference's
construct_graph (tests/cloud_restate.py).  The kernel itself is checked in test_gpu_cloud_fps.py."""
import os
import re

import numpy as np
import pytest
import torch

import cloud_restate as CR
from adaptigraph_amd import perception as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_and_the_abi_version_stays():
    import adaptigraph_amd as ag
    from adaptigraph_amd import _lib
    src = open(os.path.join(ROOT, "include", "adaptigraph_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+ag_fps_cloud\s*\(", code)
    assert re.search(r"#define\s+AG_ABI_VERSION\s+7u?\b", code)
    assert "ag_fps_cloud" in _lib.EXPORTS
    for name in ("perception", "fps_cloud", "construct_graph", "state_cur_from_points"):
        assert name in ag.__all__ and hasattr(ag, name)
    # both entries take the same arguments
    args = lambda fn: re.sub(r"\s+", " ", re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % fn, code, flags=re.S).group(1))   # noqa: E731
    assert args("ag_fps_cloud") == args("ag_fps_batch")


def test_python_constants_are_the_kernel_s():
    """The sizes the GPU tests are built around (workgroup, register / workspace switch, limit) are the ones compiled in."""
    hip = open(os.path.join(ROOT, "adaptigraph_amd", "csrc", "ag_dataset.hip")).read()
    val = lambda name: re.search(r"constexpr int %s = ([^;]+);" % name, hip).group(1).strip()   # noqa: E731
    assert int(val("CW")) == P.CLOUD_WG
    assert val("CLOUD_S") == "CW * CLOUD_PPT" and P.CLOUD_WG * int(val("CLOUD_PPT")) == P.CLOUD_SWITCH_POINTS
    assert val("CLOUD_MAX_POINTS") == "1 << 20" and P.CLOUD_MAX_POINTS == 1 << 20


class _Shape:
    """Stands for an array of a size nobody wants to allocate: the limits are checked on shapes alone."""
    def __init__(self, *shape):
        self.shape = shape


def test_limits_are_refused_on_the_host_with_the_limit_in_the_message():
    z = torch.zeros(1, dtype=torch.int64)                   # CPU tensors: a device call would raise "no CPU fallback" instead
    with pytest.raises(NotImplementedError, match=str(P.CLOUD_MAX_POINTS)):
        P.fps_cloud(torch.zeros(4, 3), z, z, z.int(), z.float(), z.int(), 100, P.CLOUD_MAX_POINTS + 1)
    with pytest.raises(NotImplementedError, match="1024"):
        P.fps_cloud(torch.zeros(4, 3), z, z, z.int(), z.float(), z.int(), 1025, 4)
    with pytest.raises(NotImplementedError, match=str(P.CLOUD_MAX_POINTS)):
        P.construct_graph(_Shape(P.CLOUD_MAX_POINTS + 1, 3), 0.2, device="cpu", draws=[(0, 0)])
    with pytest.raises(NotImplementedError, match=str(P.CLOUD_MAX_POINTS)):
        P.state_cur_from_points(_Shape(P.CLOUD_MAX_POINTS + 1, 3), 10, device="cpu", draws=[(0, 0)])


def test_argument_errors_come_before_any_device_call():
    cloud = np.zeros((50, 3), np.float32)
    with pytest.raises(NotImplementedError, match="visualize"):
        P.construct_graph(cloud, 0.2, visualize=True, device="cpu", draws=[(0, 0)])
    with pytest.raises(ValueError, match="max_neef 8"):
        P.construct_graph(cloud, 0.2, eef_kps=np.zeros((9, 3), np.float32), device="cpu", draws=[(0, 0)])
    with pytest.raises(ValueError, match="exceed max_nobj 100"):        # known after the read-back of the counts: the layout refuses
        P.graph_layout([60, 41], 0, 100, 8)
    with pytest.raises(ValueError, match="non-empty"):
        P.construct_graph([cloud, np.zeros((0, 3), np.float32)], 0.2, device="cpu", draws=[(0, 0), (0, 0)])
    with pytest.raises(ValueError, match="pairs for 2 objects"):
        P.construct_graph([cloud, cloud], 0.2, device="cpu", draws=[(0, 0)])
    with pytest.raises(ValueError, match="outside"):
        P.construct_graph(cloud, 0.2, max_nobj=10, device="cpu", draws=[(0, 10)])
    with pytest.raises(ValueError, match="outside"):
        P.construct_graph(cloud, 0.2, device="cpu", draws=[(50, 0)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # all arguments fine: only now the device is asked for
        P.construct_graph(cloud, 0.2, device="cpu", draws=[(0, 0)])


def test_default_draws_consume_numpy_s_generator_as_the_reference_does():
    """perception.py:271 draws np.random.randint(0, n) per object, then fps_rad_idx (utils.py:14) np.random.randint(n1) on the
    stage-1 points, object after object."""
    sizes, max_nobj = [20000, 37, 300], 100
    np.random.seed(1234)
    want = []
    for n in sizes:
        a = np.random.randint(0, n)
        want.append((a, np.random.randint(min(max_nobj, n))))
    after = np.random.randint(1 << 30)
    np.random.seed(1234)
    got = P.draw_starts(sizes, max_nobj)
    assert got == want and np.random.randint(1 << 30) == after           # exactly two draws per object, nothing else consumed
    np.random.seed(1234)                                                 # the argument check is what construct_graph calls
    assert P._check_graph_args(sizes, [(n, 3) for n in sizes], 0, max_nobj, 8, False, None) == want
    np.random.seed(1234)                                                 # explicit draws leave the generator alone
    P._check_graph_args(sizes, [(n, 3) for n in sizes], 0, max_nobj, 8, False, [(0, 0)] * 3)
    assert np.random.randint(0, sizes[0]) == want[0][0]


@pytest.mark.parametrize("sizes,n_eef,radius", [((400,), 0, 0.2), ((400,), 3, 0.35), ((900, 40), 2, 0.45), ((30, 25), 8, 0.0)])
def test_layout_equals_the_restated_construct_graph(sizes, n_eef, radius):
    """graph_layout's row ranges and masks against the restatement, for one object and for two."""
    rng = np.random.default_rng(len(sizes) + n_eef)
    clouds = [(rng.normal(size=(n, 3)) * [1.0, 0.1, 0.6]).astype(np.float32) + 3 * j for j, n in enumerate(sizes)]
    eef = rng.normal(size=(n_eef, 3)).astype(np.float32) if n_eef else None
    draws = [(int(rng.integers(n)), int(rng.integers(min(100, n)))) for n in sizes]
    want = CR.construct_graph(clouds if len(clouds) > 1 else clouds[0], radius, draws, eef_kps=eef)
    counts = [len(i) for i in want["fps_idx_list"]]
    assert sum(counts) <= 100
    lay = P.graph_layout(counts, n_eef)
    assert lay["obj_kp_num"] == len(want["obj_state_raw"]) == sum(counts)
    assert np.array_equal(lay["state_mask"], want["state_mask"]) and np.array_equal(lay["eef_mask"], want["eef_mask"])
    state = np.zeros((108, 3), np.float32)
    for c, idx, (r0, r1) in zip(clouds, want["fps_idx_list"], lay["rows"]):
        assert r1 - r0 == len(idx)
        state[r0:r1] = c[idx]
    if n_eef:
        state[100:100 + n_eef] = eef
    assert np.array_equal(state.view(np.uint32), want["state"].view(np.uint32))
    assert lay["rows"][0][0] == 0 and all(a[1] == b[0] for a, b in zip(lay["rows"], lay["rows"][1:]))
