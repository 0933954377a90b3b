"""The switches of the 3x3 convolution dispatch select other kernels for the same launches (Winograd off / wherever eligible, the
direct LDS-DMA kernels with wave priorities, the register-staged kernels).  They are not defaults, but they are compiled in and some
inputs reach those kernels only: each must still give the right numbers (tools/knob_check.py: plain torch on the CPU as the
reference, batch 64, NaN-poisoned LDS)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The Winograd kernels (TG_CONV_WINO, default 1) take the stride-1 3x3 launches that fill the chip and the >= 32-channel pooled
# convolutions; the direct kernels behind them run with TG_CONV_WINO=0.
_DIRECT = [{'TG_DMA_PRIO': '1'}, {'TG_CONV_DMA': '0'}]
KNOBS = [{}, {'TG_CONV_WINO': '0'}, {'TG_CONV_WINO': '2'}] + [dict(k, TG_CONV_WINO='0') for k in _DIRECT]


@pytest.mark.parametrize('knobs', KNOBS, ids=lambda k: ','.join(f'{a[3:]}={b}' for a, b in k.items()) or 'defaults')
def test_kernels_under_knob(knobs):
    env = dict(os.environ, **knobs)
    r = subprocess.run([sys.executable, os.path.join(REPO, 'tools', 'knob_check.py')], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
