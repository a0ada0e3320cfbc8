"""CPU checks of tests/set_loss_edges.py: the restated rule of the set-loss kernels is right (the reference's recordings in
tests/golden/set_losses.npz; torch in float64 on the boundary, tie and non-finite cases), its one known difference from torch - the
gradient at an exactly tied maximum - is on record, every case meets the conditions it was built under, and every mutant of the rule
is told apart by a named case.  Nothing here needs the library or a GPU."""
import numpy as np
import pytest
import torch

import set_loss_edges as E
import set_loss_restate as SR
from test_set_losses import standalone_cases, SHAPES


def _autograd(fn, x, y, grad_out=1.0):
    xt = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    v = fn(xt, torch.from_numpy(np.asarray(y, np.float64)))
    (grad_out * v).backward()
    return float(v.detach()), xt.grad.numpy()


FN = {"chamfer": SR.chamfer, "hausdorff": SR.hausdorff}


# ------------------------------------------------------------------------------------------------ the yardstick is right
@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_rule_reproduces_the_recorded_reference(k):
    c = standalone_cases()[k]
    for kind in ("chamfer", "hausdorff"):
        for dt in (np.float64, np.float32):
            r = E.set_rule(c["x"], c["y"], dt, kind)
            ref, g_ref = float(c[kind]), c["g_" + kind]
            assert abs(r["value"] - ref) <= 1e-5 * abs(ref), (kind, dt, r["value"], ref)
            assert np.isfinite(r["grad"]).all()
            assert np.abs(r["grad"] - g_ref).max() <= 1e-4 * np.abs(g_ref).max() + 1e-7, (kind, dt)
        r = E.set_rule(c["x"], c["y"], np.float64, kind)
        assert abs(r["value"] - float(c[kind + "_64"])) <= 1e-12 * abs(float(c[kind + "_64"]))
        ax, ay, bx, by = SR.winners(c["x"].astype(np.float64), c["y"].astype(np.float64))
        N, M = SHAPES[k][1:]
        assert np.array_equal(r["nnx"], ax) and np.array_equal(r["nny"], ay) and r["win"] == [bx // N, bx % N, by // M, by % M]


@pytest.mark.parametrize("shape", E.BOUNDARY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_rule_equals_float64_autograd_on_the_boundary_cases(shape):
    x, y, seed = E.boundary_case(*shape)
    gaps = SR.gaps(x, y)
    print(f"boundary {shape}: seed {seed}, gaps {gaps.tolist()}")
    assert (gaps >= E.GAP_BAR).all()                                        # the condition the case was built under
    for kind in ("chamfer", "hausdorff"):
        r = E.set_rule(x, y, np.float64, kind, grad_out=3.0)
        v, g = _autograd(FN[kind], x, y, 3.0)
        assert abs(r["value"] - v) <= 1e-12 * abs(v), (kind, r["value"], v)
        assert np.abs(r["grad"] - g).max() <= 1e-12 * np.abs(g).max(), kind
        r32 = E.set_rule(x, y, np.float32, kind)
        assert np.array_equal(r["nnx"], r32["nnx"]) and np.array_equal(r["nny"], r32["nny"]) and r["win"] == r32["win"]


def test_chunked_rule_equals_the_unchunked_one(monkeypatch):
    x, y, _ = E.boundary_case(2, 100, 157)
    whole = E.set_rule(x, y, np.float64, "chamfer", want_gaps=True)
    monkeypatch.setattr(E, "CHUNK_ELEMS", 157 * 7)                           # chunks of 7 rows: 100 and 157 are no multiples
    parts = E.set_rule(x, y, np.float64, "chamfer", want_gaps=True)
    for k in ("nnx", "nny", "grad", "gx", "gy"):
        assert np.array_equal(whole[k], parts[k]), k
    assert whole["value"] == parts["value"] and whole["win"] == parts["win"]
    g = SR.gaps(x, y)
    assert min(whole["gx"].min(), whole["gy"].min()) == pytest.approx(min(g[0], g[1]), rel=0, abs=1e-15)


# ------------------------------------------------------------------------------------------------ ties and non-finite: torch's values
def _torch_tables(x, y):
    """what torch.min(dim) and torch.max give in float64 on the CPU: minima, their indices, the two maxima and their flat places"""
    dis = SR.pair_dist(torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(y, np.float64)))
    mx, ax = dis.min(dim=2)
    my, ay = dis.min(dim=1)
    return mx, ax.numpy(), my, ay.numpy()


def _same_as_torch(name, x, y):
    r = {k: E.set_rule(x, y, np.float64, k) for k in ("chamfer", "hausdorff")}
    mx, ax, my, ay = _torch_tables(x, y)
    assert np.array_equal(r["chamfer"]["nnx"], ax) and np.array_equal(r["chamfer"]["nny"], ay), name
    ch, hd = float(mx.mean() + my.mean()), float(mx.max() + my.max())
    for kind, ref in (("chamfer", ch), ("hausdorff", hd)):
        v = r[kind]["value"]
        assert (np.isnan(v) and np.isnan(ref)) or v == ref or abs(v - ref) <= 1e-12 * abs(ref), (name, kind, v, ref)
    bx, i, by, j = r["hausdorff"]["win"]                                   # the winners hold torch's maxima
    assert E.same_float(mx[bx, i], mx.max()) and E.same_float(my[by, j], my.max()), name
    return r


@pytest.mark.parametrize("kind", E.TIE_KINDS)
def test_tie_cases_give_torchs_values_and_indices(kind):
    c = E.tie_case(kind)
    x, y = c["x"], c["y"]
    r = _same_as_torch(kind, x, y)
    ch, hd = r["chamfer"], r["hausdorff"]
    for b, i, j in c["expect"].get("nnx", []):
        assert ch["nnx"][b, i] == j
    for b, j, i in c["expect"].get("nny", []):
        assert ch["nny"][b, j] == i
    for k, w in c["expect"].get("win", []):
        assert hd["win"][k] == w, (kind, hd["win"])
    if "value" in c["expect"]:
        assert ch["value"] == c["expect"]["value"] == hd["value"]
        assert not ch["grad"].any() and not hd["grad"].any()
    for name in ("chamfer", "hausdorff"):                                   # fp32 and float64 decide alike
        r32 = E.set_rule(x, y, np.float32, name)
        assert np.array_equal(r[name]["nnx"], r32["nnx"]) and np.array_equal(r[name]["nny"], r32["nny"]) and r[name]["win"] == r32["win"]
    # the Chamfer gradient is torch's wherever the arg-min is torch's: everywhere
    v, g = _autograd(SR.chamfer, x, y)
    assert np.abs(ch["grad"] - g).max() <= 1e-12 * max(np.abs(g).max(), 1e-300), kind
    v, g = _autograd(SR.hausdorff, x, y)
    diff = np.abs(hd["grad"] - g).max()
    if not c["tied"]:
        assert diff <= 1e-12 * max(np.abs(g).max(), 1e-300), kind
        return
    # THE KNOWN DIFFERENCE.  torch.max() over the batch splits its gradient evenly among the equal maxima; the rule (and the
    # kernel) gives the whole weight to the lowest (b, index).  The tied rows together carry the same pull either way.
    rows = np.array(c["tied"])
    n = len(rows)
    g_tied, r_tied = g[rows[:, 0], rows[:, 1]], hd["grad"][rows[:, 0], rows[:, 1]]
    unit = np.linalg.norm(r_tied[0])
    print(f"tie {kind}: {n} equal maxima; autograd gives each {np.linalg.norm(g_tied, axis=1).tolist()}, the rule gives row "
          f"{tuple(rows[0])} {unit:.6f} and the others 0; largest difference {diff:.6f}")
    assert unit > 0.99 and not r_tied[1:].any()
    assert np.allclose(np.linalg.norm(g_tied, axis=1), unit / n, rtol=1e-12)          # the even split
    assert diff >= (1 - 1 / n) * unit * 0.5                                            # ... is far from the rule
    assert np.abs(g_tied.sum(0) - r_tied.sum(0)).max() <= 1e-12


@pytest.mark.parametrize("kind", E.NONFINITE_KINDS)
def test_nonfinite_cases_give_torchs_values_and_indices(kind):
    c = E.nonfinite_case(kind)
    assert c["x"].shape == (3, 9, 3) and c["y"].shape == (3, 7, 3)
    r = _same_as_torch(kind, c["x"], c["y"])
    want_nan = kind != "inf_x"
    for name in ("chamfer", "hausdorff"):
        v = r[name]["value"]
        assert np.isnan(v) if want_nan else v == np.inf, (kind, name, v)
        r32 = E.set_rule(c["x"], c["y"], np.float32, name)
        assert np.array_equal(r[name]["nnx"], r32["nnx"]) and np.array_equal(r[name]["nny"], r32["nny"]) and r[name]["win"] == r32["win"]
        assert E.same_float(r32["value"], v)
        assert np.array_equal(np.isnan(r[name]["grad"]), np.isnan(r32["grad"]))
    g = r["chamfer"]["grad"]
    clean = E.set_rule(c["x0"], c["y0"], np.float64, "chamfer")["grad"]
    good = [b for b in range(3) if b not in c["bad"]]
    assert np.array_equal(g[good], clean[good])                             # a clean graph never sees the other's NaN
    for b, i in c["nan_rows"]:
        assert np.isnan(g[b, i]).any()
    # every row the rule makes NaN is NaN under torch's autograd as well, which forms the whole (N, M) matrix and so spreads
    # 0 * NaN over more rows of the same graph (all nine with inf - inf); the clean graphs stay clean there too
    _, gt = _autograd(SR.chamfer, c["x"], c["y"])
    nan_rule, nan_torch = np.isnan(g).any(2), np.isnan(gt).any(2)
    assert (nan_torch | ~nan_rule).all() and not nan_torch[good].any(), kind


def test_the_fused_batch_is_the_first_admitted_seed():
    for seed in range(E.FUSED_SEED + 1):
        ok, gaps, sens = E.fused_qualifies(seed)
        print(f"fused batch seed {seed}: admitted {ok}, chain gaps per step {gaps.tolist()}, rounding sensitivity {sens}")
        assert ok == (seed == E.FUSED_SEED)
    assert (gaps >= E.GAP_BAR).all() and sens <= E.FUSED_SENSITIVITY
    bt = E.fused_batch(E.FUSED_SEED)
    c = E.FUSED
    assert bt["state_future"].shape == (c["B"], c["n_future"], c["n_p"], 3) and c["n_p"] + 1 == c["N"] == 258
    assert all(len(r) == c["per_recv"] * c["N"] for r in bt["recv_l"])


# ------------------------------------------------------------------------------------------------ the cases bite
def test_every_mutant_is_told_apart_by_a_named_case():
    cases = E.named_cases()
    rule = {(n, k, dt): E.set_rule(x, y, dt, k, B_total=bt) for n, (x, y, bt) in cases.items() for k in ("chamfer", "hausdorff")
            for dt in (np.float64, np.float32) if not (k == "hausdorff" and bt is not None)}
    missed = []
    for m in E.MUTANTS:
        caught = {}
        for n, (x, y, bt) in cases.items():
            for k in ("chamfer", "hausdorff"):
                if (n, k, np.float64) not in rule:
                    continue
                why = E.told_apart(rule[n, k, np.float64], rule[n, k, np.float32], E.set_rule(x, y, np.float64, k, B_total=bt, mutant=m))
                if why:
                    caught.setdefault(n, []).append(f"{k}: {why}")
        print(f"MUTANT {m}: caught by " + ("; ".join(f"{n} ({', '.join(w)})" for n, w in caught.items()) or "NOTHING"))
        if not caught:
            missed.append(m)
    assert not missed, missed


def test_the_rule_is_not_told_apart_from_itself():
    for n, (x, y, bt) in E.named_cases().items():
        a, a32 = E.set_rule(x, y, np.float64, "chamfer", B_total=bt), E.set_rule(x, y, np.float32, "chamfer", B_total=bt)
        assert E.told_apart(a, a32, E.set_rule(x, y, np.float64, "chamfer", B_total=bt)) is None, n
        assert E.told_apart(a, a32, a32 | {"grad": a32["grad"].astype(np.float64)}) is None, n   # nor is fp32 rounding
