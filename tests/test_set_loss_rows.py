"""CPU checks of tests/set_loss_rows.py, the rule of the set losses over each graph's real rows (AG_LOSS_ROWS): it reproduces the
reference's recordings of the sliced graphs (tests/golden/set_losses_rows.npz), at full counts it is the plain rule (set_rule,
emd_restate), every mutant is told apart by a named case, and the host side - LossSpec(real_rows=True), the constant, the header's
text, the export count - is what the issue fixed.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest

import emd_restate as ER
import set_loss_edges as SE
import set_loss_rows as RW

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def fixture():
    return dict(np.load(os.path.join(HERE, "golden", "set_losses_rows.npz")))


def batch(f, tag):
    return {k.split("::", 1)[1]: v for k, v in f.items() if k.startswith(tag + "::")}


BATCHES = {"a": RW.BATCH_A, "b": RW.BATCH_B}


# ------------------------------------------------------------------------------------------------ the yardstick is right
@pytest.mark.parametrize("tag", ["a", "b"])
def test_fixture_is_what_the_generator_promises(tag):
    f = fixture()
    c, spec = batch(f, tag), BATCHES[tag]
    assert c["x"].shape == (spec["B"], spec["N"], 3) and c["y"].shape == (spec["B"], spec["M"], 3)
    assert c["nx"].tolist() == spec["nx"] and c["ny"].tolist() == spec["ny"]
    rec = c["recorded"]
    assert rec.tolist() == [n > 0 and m > 0 for n, m in zip(spec["nx"], spec["ny"])]
    assert int((~rec).sum()) == (2 if tag == "a" else 0)                     # the reference cannot evaluate an empty side
    assert (c["nn_gaps"][rec][:, :2] >= float(f["nn_gap_bar"])).all() and (c["emd_gap"][rec] >= float(f["emd_gap_bar"])).all()
    assert float(f["nn_gap_bar"]) == 1e-4 and float(f["emd_gap_bar"]) == 1e-4
    for b in range(spec["B"]):                                               # zero padding, as the loader writes it
        assert not c["x"][b, spec["nx"][b]:].any() and not c["y"][b, spec["ny"][b]:].any()
    assert RW.qualifies(c["x"], c["y"], c["nx"], c["ny"])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_rule_reproduces_the_recorded_reference_graph_by_graph(tag):
    """every recorded graph as a batch of one: the rule over its real rows is the reference's module on the slice"""
    c = batch(fixture(), tag)
    for b in np.nonzero(c["recorded"])[0]:
        xb, yb, n, m = c["x"][b:b + 1], c["y"][b:b + 1], c["nx"][b:b + 1], c["ny"][b:b + 1]
        for kind, key in (("chamfer", "chamfer"), ("hausdorff", "hausdorff"), ("earth_mover", "emd")):
            for dt in (np.float64, np.float32):
                r = RW.rows_rule(xb, yb, n, m, dt, kind)
                ref, g_ref = float(c[key][b]), c["g_" + key][b]
                assert abs(r["value"] - ref) <= 1e-5 * abs(ref), (tag, b, kind, dt, r["value"], ref)
                assert np.abs(r["grad"][0] - g_ref).max() <= 1e-4 * np.abs(g_ref).max() + 1e-7, (tag, b, kind, dt)
                assert not r["grad"][0, n[0]:].any()
            r = RW.rows_rule(xb, yb, n, m, np.float64, kind)
            assert abs(r["value"] - float(c[key + "_64"][b])) <= 1e-12 * abs(float(c[key + "_64"][b])), (tag, b, kind)
        r = RW.rows_rule(xb, yb, n, m, np.float64, "earth_mover")
        assert np.array_equal(r["ind1"][0], c["ind1"][b]) and np.array_equal(r["ind2"][0], c["ind2"][b])
        assert abs(RW.rows_rule(xb, yb, n, m, np.float64, "chamfer")["value"] - c["mean_chamfer"][b]) <= 1e-12


@pytest.mark.parametrize("tag", ["a", "b"])
def test_batch_values_are_the_means_over_graphs_of_the_recordings(tag):
    """Chamfer = mean_chamfer(...).mean() with an empty graph adding 0 and counting in B; Earth-mover likewise; Hausdorff the sum of
    the per-side maxima, which bounds every recorded graph's own value from above and equals one of them when both sit in one graph"""
    c = batch(fixture(), tag)
    B, rec = len(c["nx"]), c["recorded"]
    r = {k: RW.rows_rule(c["x"], c["y"], c["nx"], c["ny"], np.float64, k) for k in RW.KINDS}
    assert abs(r["chamfer"]["value"] - c["mean_chamfer"][rec].sum() / B) <= 1e-12
    assert abs(r["chamfer"]["value"] - c["chamfer_64"][rec].sum() / B) <= 1e-12
    assert abs(r["earth_mover"]["value"] - c["emd_64"][rec].sum() / B) <= 1e-12
    hd, win = r["hausdorff"]["value"], r["hausdorff"]["win"]
    assert (hd >= c["hausdorff_64"][rec] - 1e-12).all() and rec[win[0]] and rec[win[2]]
    if win[0] == win[2]:
        assert abs(hd - c["hausdorff_64"][win[0]]) <= 1e-12
    # gradients: a graph's rows are the recorded ones over B (Chamfer, Earth-mover); rows of padding and of empty graphs are zero
    for kind, key in (("chamfer", "g_chamfer"), ("earth_mover", "g_emd")):
        g = r[kind]["grad"]
        assert np.abs(g - c[key] / B).max() <= 1e-6 * np.abs(c[key]).max(), kind
        for b in range(B):
            assert not g[b, r[kind]["nx"][b]:].any()
    assert np.array_equal(r["earth_mover"]["ind1"], c["ind1"]) and np.array_equal(r["earth_mover"]["ind2"], c["ind2"])


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 7, 5), (2, 5, 7), (2, 70, 37)], ids=lambda s: "x".join(map(str, s)))
def test_full_counts_are_the_plain_rule(shape):
    B, N, M = shape
    x, y, _ = RW.case(B, N, M, [N] * B, [M] * B)
    full = ([N] * B, [M] * B)
    for kind in ("chamfer", "hausdorff"):
        for counts in (full, ([N + 5] * B, [M + 1] * B)):                    # counts above the size are clamped
            r, p = RW.rows_rule(x, y, *counts, np.float64, kind, grad_out=3.0), SE.set_rule(x, y, np.float64, kind, grad_out=3.0)
            assert np.array_equal(r["nnx"], p["nnx"]) and np.array_equal(r["nny"], p["nny"]) and r["win"] == p["win"]
            assert abs(r["value"] - p["value"]) <= 1e-14 * abs(p["value"]) and (kind != "hausdorff" or r["value"] == p["value"])
            assert np.abs(r["grad"] - p["grad"]).max() <= 1e-14 * np.abs(p["grad"]).max()
    r = RW.rows_rule(x, y, *full, np.float64, "earth_mover", grad_out=3.0)
    i1, i2 = ER.assignment(x, y)
    v, g = ER.value_and_grad(x, y, i1, i2)
    assert np.array_equal(r["ind1"], i1) and np.array_equal(r["ind2"], i2)
    assert abs(r["value"] - v) <= 1e-14 * abs(v) and np.abs(r["grad"] - 3.0 * g).max() <= 1e-13 * np.abs(g).max()


def test_empty_graphs_and_clamped_counts():
    x, y, _ = RW.case(4, 6, 5, [0, 4, 6, 0], [5, 0, 3, 0])
    for kind in RW.KINDS:
        r = RW.rows_rule(x, y, [0, 4, 6, 0], [5, 0, 3, 0], np.float64, kind)
        one = RW.rows_rule(x[2:3], y[2:3], [6], [3], np.float64, kind)
        assert np.isfinite(r["value"]) and not r["grad"][[0, 1, 3]].any()
        # the empty graphs count in B: a mean is the lone live graph's over 4; a max is the lone live graph's
        assert abs(r["value"] - one["value"] / (1 if kind == "hausdorff" else 4)) <= 1e-15
        same = RW.rows_rule(x, y, [-3, 4, 99, 0], [5, -1, 3, 0], np.float64, kind)
        assert same["value"] == r["value"] and np.array_equal(same["grad"], r["grad"])
        none = RW.rows_rule(x, y, [0] * 4, [0] * 4, np.float64, kind)
        assert none["value"] == 0.0 and not none["grad"].any() and none["win"] == [-1] * 4
    assert RW.rows_rule(x, y, [0, 4, 6, 0], [5, 0, 3, 0], kind="hausdorff")["win"][0] == 2


def test_padding_is_never_read():
    c = batch(fixture(), "a")
    for kind in RW.KINDS:
        r0 = RW.rows_rule(c["x"], c["y"], c["nx"], c["ny"], np.float32, kind, want_gaps=False)
        for fill in (np.nan, np.inf, 1e30):
            x, y = RW.with_padding(c["x"], c["y"], c["nx"], c["ny"], fill)
            r = RW.rows_rule(x, y, c["nx"], c["ny"], np.float32, kind)
            assert r["value"] == r0["value"] and np.array_equal(r["grad"], r0["grad"]) and np.array_equal(r["nnx"], r0["nnx"])


# ------------------------------------------------------------------------------------------------ the mutants
def _hausdorff_trap():
    """batch a with a padding row of x far away: it would win the plain max"""
    c = batch(fixture(), "a")
    x = c["x"].copy()
    x[1, 7] = SE.FAR_P                                                       # nx[1] = 5: row 7 is padding
    return x, c["y"], c["nx"], c["ny"]


def mutant_cases():
    """name -> (x, y, nx, ny, kind): the named case every mutant must be caught by"""
    a = batch(fixture(), "a")
    xa, ya, nxa, nya = a["x"], a["y"], a["nx"], a["ny"]
    live = ([9, 5, 1, 9, 9, 3], [7, 7, 2, 4, 7, 3])                          # batch a without empty graphs, N != M
    return {
        "denominator_padded": ("batch a chamfer", xa, ya, nxa, nya, "chamfer"),
        "pooled_mean": ("batch a chamfer", xa, ya, nxa, nya, "chamfer"),
        "pad_rows_searched": ("batch a chamfer: the padding at the origin is some real row's nearest", xa, ya, nxa, nya, "chamfer"),
        "pad_grad_nonzero": ("batch a chamfer", xa, ya, nxa, nya, "chamfer"),
        "counts_swapped": ("batch a without empty graphs, chamfer", xa, ya, *live, "chamfer"),
        "empty_is_nan": ("batch a chamfer", xa, ya, nxa, nya, "chamfer"),
        "emd_K_padded": ("batch a earth_mover", xa, ya, nxa, nya, "earth_mover"),
        "hausdorff_pad_wins": ("batch a with a far padding row, hausdorff", *_hausdorff_trap(), "hausdorff"),
    }


@pytest.mark.parametrize("mutant", RW.MUTANTS)
def test_every_mutant_is_told_apart_by_its_named_case(mutant):
    name, x, y, nx, ny, kind = mutant_cases()[mutant]
    r64, r32 = (RW.rows_rule(x, y, nx, ny, dt, kind, grad_out=3.0) for dt in (np.float64, np.float32))
    assert RW.told_apart(r64, r32, r64) is None and RW.told_apart(r64, r32, r32) is None
    why = RW.told_apart(r64, r32, RW.rows_rule(x, y, nx, ny, np.float64, kind, grad_out=3.0, mutant=mutant))
    print(f"{mutant}: caught by '{name}' through its {why}")
    assert why is not None, (mutant, name)


def test_mutant_list_is_the_issue_s():
    assert set(RW.MUTANTS) == {"denominator_padded", "pooled_mean", "pad_rows_searched", "pad_grad_nonzero", "counts_swapped",
                               "empty_is_nan", "emd_K_padded", "hausdorff_pad_wins"}
    assert set(mutant_cases()) == set(RW.MUTANTS)


# ------------------------------------------------------------------------------------------------ the host side
def test_loss_spec_real_rows_flags_the_set_terms_only():
    import torch
    from adaptigraph_amd import _lib
    from adaptigraph_amd.set_losses import LossSpec, ChamferLoss, HausdorffLoss, EarthMoverLoss
    R = _lib.AG_LOSS_ROWS
    terms = [("mse", 1.0), (ChamferLoss(), 0.5), ("hausdorff", 0.25), (EarthMoverLoss(), 2.0)]
    plain, rows = LossSpec(terms), LossSpec(terms, real_rows=True)
    assert plain.kinds == [0, 1, 2, 3] and rows.kinds == [0, 1 | R, 2 | R, 3 | R]
    assert rows.names == plain.names and rows.weights == plain.weights and rows.has_hausdorff and plain.has_hausdorff
    assert LossSpec(terms, real_rows=False).kinds == plain.kinds and not LossSpec([("mse", 1), ("chamfer", 1)], real_rows=True).has_hausdorff
    s = rows.c_struct()
    assert s.n_terms == 4 and list(s.kind) == rows.kinds
    with pytest.raises(ValueError, match="does not split"):
        rows.forbid_parts("accumulate")
    LossSpec([("mse", 1), ("chamfer", 1), (EarthMoverLoss(), 1)], real_rows=True).forbid_parts("accumulate")     # the means split
    assert LossSpec(None, real_rows=True).default and LossSpec(None, real_rows=True).kinds == [0]
    # nothing new is rejected, nothing old accepted
    for bad in ([("emd", 1)], [("nope", 1)], [("chamfer", float("nan"))], []):
        for kw in ({}, {"real_rows": True}):
            with pytest.raises((ValueError, NotImplementedError)):
                LossSpec(bad, **kw)
    assert LossSpec([(torch.nn.MSELoss(), 1), (HausdorffLoss(), 1)], real_rows=True).kinds == [0, 2 | R]


def test_prefix_counts_on_the_host():
    import torch
    from adaptigraph_amd.set_losses import prefix_counts
    m = torch.tensor([[1, 1, 1, 1], [1, 1, 0, 1], [0, 1, 1, 1], [0, 0, 0, 0]])
    for mask in (m.bool(), m.to(torch.uint8)):
        n = prefix_counts(mask)
        assert n.dtype == torch.int32 and n.tolist() == [4, 2, 0, 0]
    with pytest.raises(AssertionError):
        prefix_counts(m.float())


def test_header_constant_and_exports():
    from adaptigraph_amd import _lib
    h = open(os.path.join(ROOT, "include", "adaptigraph_amd.h")).read()
    assert re.search(r"^#define AG_LOSS_ROWS 16\b", h, re.M) and _lib.AG_LOSS_ROWS == 16
    assert re.search(r"^#define AG_ABI_VERSION 7\b", h, re.M) and len(_lib.EXPORTS) == 51
    text = " ".join(h.split())
    assert "B*(N+M) + 4 + 2B int32" in text and "nx[0..B) then ny[0..B)" in text and "REQUIRED" in text
    assert "No masks" not in h
    assert (_lib.AG_LOSS_MSE, _lib.AG_LOSS_CHAMFER, _lib.AG_LOSS_HAUSDORFF, _lib.AG_LOSS_EMD) == (0, 1, 2, 3)
