"""GPU: tools/run_greens.py end to end, in a child process of its own -- a 2 x 3 lattice of SST patches, a control and the
sum pattern as one eight-member engine for one year, three of the patches again as one-member engines (--compare: bit
equality or a non-zero exit status)."""
import json
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_greens_small_lattice_with_compare():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "run_greens.py"), "2", "3", "1", "--compare"], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    print(r.stdout)
    m = re.search(r"^additivity ratio: (\S+)$", r.stdout, re.M)
    assert m, out[-3000:]
    assert math.isfinite(float(m.group(1)))
    assert len(re.findall(r"^compare: patch \d+ as a one-member engine equals member", r.stdout, re.M)) == 3
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["members"] == 8 and d["finite"] and d["describe"]["sst"] == {"patterns": 7, "prescribed_members": 8}
    assert all(c["bit_equal"] for c in d["compare"]) and len(d["compare"]) == 3
