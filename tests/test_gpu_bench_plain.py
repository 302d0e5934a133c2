"""-m gpu: a plain `bench.py --gpus 1 --steps K --warmup W` prints the headline line and nothing else, and --dump-outputs writes the
y that its timed launches computed (checked against the same seeded layer, dequantised and multiplied densely)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("steps,warmup", [(7, 3), (300, 20)])          # eager launches behind a spin kernel / one hipGraph
def test_plain_run_prints_the_headline_and_dumps_y(tmp_path, steps, warmup):
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                         "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr[-2000:]
    lines = [l for l in pr.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, pr.stdout
    out = json.loads(lines[0])
    assert out["steps"] == steps and out["warmup"] == warmup and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["unit"] == "TFLOP/s" and out["higher_is_better"] is True and out["dtype"] == "bf16" and "metric" in out
    for k in ("parity_rel_err", "from_idle", "warm", "fp32_y", "accumulate_contract", "k2_shapes", "sharded_ldlq", "decode", "cpu_baseline"):
        assert k not in out, k                                                  # --full only

    sys.path.insert(0, ROOT)
    import bench
    from quip_amd import ops
    y = np.load(tmp_path / "y.npy")
    assert y.dtype == np.float32 and y.shape == (bench.BS, bench.M)
    torch.manual_seed(0)                                                        # bench.py's set-up
    W = (0.02 * torch.randn(bench.M, bench.D)).to(DEV)
    scale = ops.qfnb_scale(W)
    _, codes = ops.quantize(W, "b", scale, None, bench.MAXQ, want_codes=True)
    x = torch.randn(bench.BS, bench.D).to(torch.bfloat16)
    What = ops.codes_to_weight(codes, "b", scale, None, bench.MAXQ, out_dtype=torch.float32).cpu()
    ref = (x.double() @ What.double().T).numpy()
    rel = np.linalg.norm(y - ref) / np.linalg.norm(ref)
    assert rel < 5e-3, rel                                                      # smoke()'s bound for y rounded to bf16
