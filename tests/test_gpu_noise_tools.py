"""GPU: tools/run_noise.py end to end, in a child process of its own -- four noisy members and a noise-free one as one
five-member engine for two years through run_ens and run_diag; --compare: the heat flux against the numpy mirror and the
noise-free member against a plain one-member engine, bit equality or a non-zero exit status."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_noise_small_ensemble_with_compare():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_noise.py"), "4", "2", "--compare"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    print(r.stdout)
    assert re.search(r"^compare: the noise-free member equals a plain one-member engine \(default kernels\)$", r.stdout, re.M), out[-3000:]
    assert len(re.findall(r"^compare: N of member 0 at step \d+: .* equal bit for bit$", r.stdout, re.M)) == 2
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["members"] == 5 and d["noisy"] == 4 and d["finite"] and d["describe"]["noise"] == {"patterns": 1, "noisy_members": 4}
    assert d["std_december_tsurf_K"]["ocean"] > 0 and d["std_annual_tsurf_K"]["ocean"] > 0
    assert d["std_december_tsurf_K"]["land"] > 0 and d["std_annual_tsurf_K"]["land"] > 0
    assert -1.0 <= d["lag1_year_autocorrelation"] <= 1.0 and d["member_years_per_s"] > 0
    assert d["compare"]["plain_bit_equal"] and all(c["bit_equal"] for c in d["compare"]["noise"])
    for c in d["compare"]["noise"]:  # sigma 30 W/m2 over ocean, 10 over land: the flux's RMS over a few thousand cells is near them
        assert 20.0 < c["device_rms_ocean_land"][0] < 40.0 and 5.0 < c["device_rms_ocean_land"][1] < 15.0
