"""sfm_xcorr_workspace_bytes: the sizes and refusals of every correlation path.

The call makes no HIP call and dereferences nothing, so these run without a GPU
on descriptors with fixed fake addresses.  The expected byte counts and messages
in tests/golden/xcorr_workspace.json were recorded once from the library of the
commit before the driver got its single plan (tests/golden/make_golden_xcorr_workspace.py):
a workspace that changes size changes what `flow_field` allocates per call and
whether a whole pair still fits one launch.
"""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
sys.path.insert(0, GOLDEN)
from make_golden_xcorr_workspace import measure  # noqa: E402

with open(os.path.join(GOLDEN, 'xcorr_workspace.json')) as _f:
  CASES = json.load(_f)['cases']


def test_fixture_covers_every_path_and_grouping():
  sized = [c for c in CASES if c['bytes']]
  assert {c['path'] for c in sized} == {'direct', 'fft', 'mfma', 'mfma_masked'}
  assert any(c['group'] in (0, c['batch']) for c in sized)
  assert any(0 < c['group'] < c['batch'] and c['batch'] % c['group'] for c in sized)
  assert any(c['ndim'] == 3 for c in sized)
  assert any(c.get('options') for c in sized)
  assert sum(1 for c in CASES if not c['bytes']) >= 4


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_workspace_bytes_and_refusals_are_the_recorded_ones(case):
  n, msg = measure(case)
  assert n == case['bytes']
  assert msg == case['error']
