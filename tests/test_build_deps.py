"""CPU checks of the build (adaptigraph_amd/csrc/build.sh): an object is rebuilt when a file the compiler read for it is newer or
when its command line changed, and for no other reason; the kernels' headers follow the subsystems, so a change to one of them
reaches only the files that include it."""
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "adaptigraph_amd", "csrc")
SCRIPT = os.path.join(CSRC, "build.sh")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PUBLIC = "../../include/adaptigraph_amd.h"            # as the compiler names it in the dependency files


def _dry(*args, script=SCRIPT, env=None):
    """The dry run's verdict: (objects it would compile, libraries it would link)."""
    r = subprocess.run(["bash", script, "-n", *args], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    assert all(len(ln) == 2 and ln[0] in ("compile", "link") for ln in lines), r.stdout
    return {ln[1] for ln in lines if ln[0] == "compile"}, {ln[1] for ln in lines if ln[0] == "link"}


def _objs(names, dirs=("build", "build/diag")):
    return {f"{d}/{n}.o" for d in dirs for n in names}


@pytest.fixture(scope="module")
def built():
    from adaptigraph_amd import _lib
    if not os.path.exists(_lib.LIB_PATH) or not os.path.exists(os.path.join(CSRC, "build", "diag", "ag_mlp.o")):
        import __graft_entry__ as g
        g.build()


def test_after_a_build_the_dry_run_has_nothing_to_do(built):
    assert _dry("diag") == (set(), set())
    assert _dry() == (set(), set())


def test_public_header_reaches_the_host_files_and_no_kernel_file(built):
    compiles, links = _dry("--newer", PUBLIC, "diag")
    api = [f[:-4] for f in os.listdir(CSRC) if f.startswith("ag_api") and f.endswith(".hip") and f not in ("ag_api_cma.hip", "ag_api_cells.hip")]
    assert len(api) == 6
    assert _objs(api + ["ag_dataset", "ag_eval"]) <= compiles
    assert "build/cells/ag_api_cells.o" in compiles                        # it reads ag_ctx's layout through ag_host.h
    assert not compiles & (_objs(["ag_mlp", "ag_lat", "ag_edges", "ag_graph", "ag_cost"]) | {"build/cma/ag_cma.o"})
    assert not any(os.path.basename(o) in ("ag_mlp.o", "ag_lat.o", "ag_edges.o", "ag_graph.o", "ag_cost.o", "ag_cma.o") for o in compiles)
    assert {"libadaptigraph_hip.so", "libadaptigraph_hip_diag.so", "libadaptigraph_hip_cells.so"} <= links


def test_set_loss_header_does_not_reach_the_chains(built):
    compiles, _ = _dry("--newer", "ag_setloss.h", "diag")
    assert _objs(["ag_setloss", "ag_emd", "ag_api_train"]) <= compiles
    assert not any(os.path.basename(o) in ("ag_mlp.o", "ag_lat.o") for o in compiles)


def test_model_header_reaches_the_chains_in_every_requested_variant(built):
    compiles, _ = _dry("--newer", "ag_model.h", "diag")
    assert _objs(["ag_mlp", "ag_lat"]) <= compiles
    compiles, _ = _dry("--newer", "ag_model.h")
    assert _objs(["ag_mlp", "ag_lat"], dirs=("build",)) <= compiles
    assert not any(o.startswith("build/diag/") for o in compiles)          # diag was not asked for


def test_staleness_follows_the_recorded_command_not_the_script_s_mtime(built, tmp_path):
    """A copy of the script that differs in comments only, newer than every object, run over the same tree (a directory of links,
    so the tree itself is not touched): nothing is stale.  A flag that changes the commands: everything is."""
    mirror = tmp_path / "adaptigraph_amd" / "csrc"
    mirror.mkdir(parents=True)
    os.symlink(os.path.join(ROOT, "include"), tmp_path / "include")
    for f in os.listdir(CSRC):
        if f != "build.sh":
            os.symlink(os.path.join(CSRC, f), mirror / f)
    text = open(SCRIPT).read()
    shebang, rest = text.split("\n", 1)
    (mirror / "build.sh").write_text(shebang + "\n# a comment nobody compiles\n" + rest + "\n# and one at the end\n")
    assert os.path.getmtime(mirror / "build.sh") > os.path.getmtime(os.path.join(CSRC, "build", "ag_mlp.o"))
    assert _dry("diag", script=str(mirror / "build.sh")) == (set(), set())
    assert _dry("--newer", "build.sh", "diag") == (set(), set())           # nor is the script a dependency of anything
    cmd = open(os.path.join(CSRC, "build", "ag_mlp.o.cmd")).read()
    assert "-ffp-contract=off" in cmd and "max-ilp" in cmd and cmd.rstrip().endswith("-c ag_mlp.hip -o build/ag_mlp.o")
    assert "max-ilp" not in open(os.path.join(CSRC, "build", "ag_lat.o.cmd")).read()
    compiles, links = _dry(env=dict(os.environ, AG_EXTRA_FLAGS="-DAG_A_FLAG_NOBODY_READS"))
    sources = [f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip") and f != "ag_diag.hip"]
    assert {os.path.basename(o)[:-2] for o in compiles} == set(sources) and len(compiles) == len(sources)
    assert links == {"libadaptigraph_hip.so", "libadaptigraph_hip_cma.so", "libadaptigraph_hip_cells.so"}


def test_every_header_compiles_on_its_own(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.fail(f"{HIPCC} not found: the headers cannot be checked")
    headers = sorted(f for f in os.listdir(CSRC) if f.endswith(".h"))
    assert {"ag_common.h", "ag_model.h", "ag_setloss.h", "ag_host.h", "ag_dist.h", "ag_lds_optin.h"} <= set(headers)

    def check(h):
        tu = tmp_path / (h[:-2] + "_alone.hip")
        tu.write_text(f'#include "{h}"\n')
        r = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", "-I", CSRC, str(tu)],
                           capture_output=True, text=True)
        return h, r.returncode, r.stderr

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for h, rc, err in pool.map(check, headers):
            assert rc == 0, (h, err)


def test_the_old_catch_all_header_keeps_nothing_of_a_subsystem():
    text = open(os.path.join(CSRC, "ag_common.h")).read()
    for word in ("struct", "launch_", "hipError_t", "constexpr"):
        assert word not in text, word
