"""bench.py end to end on the device: the one-GPU line (plain and --full, with the dumped outputs) and the host
side of the N > 1 path (torch.distributed replaced by a single-process stand-in, tools/smoke_bench_world2.py - no
RCCL)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(cmd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.strip().splitlines()


def test_bench_line_has_the_contract_fields():
    out = _run(["bench.py", "--n", "120", "--steps", "5", "--warmup", "1", "--full"])
    d = json.loads(out[-1])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["dtype"] == "f64" and d["vs_baseline"] is None
    assert d["roofline"]["bound"] == "hbm" and 0.0 < d["roofline"]["frac"] < 1.0
    assert d["cpu_baseline"]["kind"] == "port" and d["cpu_baseline"]["cores"] == 1
    assert d["div_residual_rel"] < 1e-10


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    """A plain run carries the headline fields of exactly K timed steps and none of the --full figures;
    --dump-outputs writes the flux of one step of the timed path, which satisfies the divergence condition."""
    out = _run(["bench.py", "--n", "120", "--steps", "7", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    d = json.loads(out[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 7 and d["dtype"] == "f64" and d["ms_per_step"] > 0.0
    assert d["value"] == pytest.approx(d["config"]["patches_per_gpu"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    for key in ("roofline", "cpu_baseline", "cold", "ms_per_step_windows", "div_residual_rel"):
        assert key not in d, key
    x = np.load(tmp_path / "flux_hdiv.npy")
    assert x.dtype == np.float64
    from dolfinx_eqlb_amd import distributed as dd
    from dolfinx_eqlb_amd.eqlb import check_eqlb_conditions as chk
    from synthetic import make_compatible_data
    part = dd.StripPartition(120, 0, 1)
    G, f = make_compatible_data(part.mesh, 2, part.facet_types(), seed=20241003)
    assert x.size == part.mesh.ncells * 8
    res, nrm = chk.divergence_residual(part.mesh, 2, x, G, f)
    assert res < 1e-10 * nrm


@pytest.mark.parametrize("rank,world,extra", [(0, 2, []), (1, 2, []), (3, 8, []), (0, 2, ["--stress"]),
                                              (0, 2, ["--k", "3"]), (1, 3, ["--ev"]), (0, 2, ["--ev", "--k", "3"])])
def test_multi_gpu_host_path(rank, world, extra):
    out = _run(["tools/smoke_bench_world2.py", "--n", "100", "--steps", "3", "--warmup", "1"] + extra,
               env={"SMOKE_RANK": str(rank), "SMOKE_WORLD": str(world)})
    if rank == 0:
        d = json.loads(out[-1])
        assert d["n_gpus"] == world and d["scaling"] == "weak"
        if not extra:
            assert "behind the interior tiles" in d["config"]["partition"]
        assert d["div_residual_rel"] < 1e-10  # rank 0 receives nothing: its owned rows (EV: held DOFs) are complete
        assert d["halo"]["rank0_bytes_sent"] > 0 and d["halo"]["halo_only_ms"] > 0.0
