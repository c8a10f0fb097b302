"""The correlation kernel's patch queue hands out runs of consecutive patches
(SFM_MFMA_RUN) -- -m gpu.

A workgroup's predictions (seed block, need mask, hot columns, the probe's
switch-off counter) carry over inside a run, so the hand-out order changes
which tiles are pruned, abandoned or redone -- never a result.  On the batch
that interleaves the seven adversarial image kinds (every prediction wrong):

* same bits as one patch per ticket (SFM_MFMA_RUN=1) and as the un-pruned run,
  at every edge of the ticket-to-patch map, with a call on other images of the
  same shapes in between (a patch nobody processed must not pass on what the
  reference call left in the workspace);
* every patch exactly once: the launch draws batch x row tiles.
"""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_prune_hardening import _interleaved_starts, _mosaic

pytestmark = pytest.mark.gpu

RUN = 4          # run length of the parametrised cases (the map's edges scale with it)
TAIL = 8         # single patches at the end of a batch, in grids (kRunTail)
ROW_TILES_48 = 6  # surface rows 48 + 48 - 1 = 95 -> six 16-row tiles


@pytest.fixture(scope='module')
def mosaics():
  return _mosaic(61), _mosaic(67)


def _call(images, size, starts):
  from sofima_amd import flow_field
  pre, post = images
  return flow_field.batched_xcorr_peaks(
      pre, post, None, None, (size, size), starts, None, method=2, min_distance=2,
      threshold_rel=0.5, peak_radius=5, post_patch_size=(size, size), post_starts=starts)


def _call_counted(images, size, starts):
  """(outputs, row tiles the correlation launch drew)."""
  from sofima_amd import _abi
  lib = _abi.load()
  pf = _abi.SfmProfile()
  lib.sfm_profile_read(C.byref(pf))
  lib.sfm_profile_enable(1)
  try:
    out = _call(images, size, starts)
    _abi.check(lib.sfm_profile_read(C.byref(pf)))
  finally:
    lib.sfm_profile_enable(0)
  return out, int(pf.tiles_drawn[0])


def _check(mosaics, size, starts, run, grid, row_tiles):
  """Reference (one patch per ticket) and un-pruned run, a call on other images,
  then the call under test with the profile hooks on."""
  from sofima_amd import _abi
  images, others = mosaics
  with _abi.option('SFM_MFMA_GRID', grid):
    with _abi.option('SFM_MFMA_RUN', 1):
      ref = _call(images, size, starts)
    with _abi.option('SFM_MFMA_PRUNE', 0):
      full = _call(images, size, starts)
    with _abi.option('SFM_MFMA_RUN', run):
      _call(others, size, starts)
      got, drawn = _call_counted(images, size, starts)
  msg = f'batch {len(starts)} grid {grid} run {run}'
  np.testing.assert_array_equal(got, ref, err_msg=msg)
  np.testing.assert_array_equal(got, full, err_msg=msg)
  assert drawn == len(starts) * row_tiles, msg


def _edge_batches(grid):
  """Batch sizes around every edge of the ticket-to-patch map for `grid`
  workgroups: fewer patches than workgroups, exactly one run each, one patch
  short of / beyond that (the run shrinks below grid x RUN), a batch that is no
  multiple of RUN, the first batch with a run queued behind the first
  assignment, and one that passes through queued runs into the single-patch
  tail."""
  full = grid * RUN
  sizes = {1, grid - 1, grid, grid + 1,
           full // 2 + 1,                  # the run shrinks to RUN / 2
           full - 1, full, full + 1,
           full + TAIL * grid - 1,         # tail cut short: first assignments stay runs
           full + TAIL * grid + RUN,       # one queued run
           full + TAIL * grid + RUN + 3,   # ... and a remainder that is no multiple of RUN
           3 * full + TAIL * grid + 1}
  return sorted(s for s in sizes if s > 0)


@pytest.mark.parametrize('grid', [1, 2, 4])
def test_runs_at_every_edge_of_the_ticket_map(gpu, mosaics, grid):
  rng = np.random.default_rng(100 + grid)
  for b in _edge_batches(grid):
    starts, _ = _interleaved_starts(rng, b, 48, 48)
    _check(mosaics, 48, starts, RUN, grid, ROW_TILES_48)


@pytest.mark.parametrize('run', [3, 8, 16])
def test_other_run_lengths_on_two_workgroups(gpu, mosaics, run):
  """Run lengths beside RUN, an odd one included, on a batch that is no multiple
  of any of them."""
  rng = np.random.default_rng(200 + run)
  starts, _ = _interleaved_starts(rng, 2 * run * 3 + 8 + 5, 48, 48)
  _check(mosaics, 48, starts, run, 2, ROW_TILES_48)


def test_whole_device_leaves_its_first_run_and_reaches_the_tail(gpu, mosaics):
  """5000 patches on the default grid with the default run length: every
  workgroup of the device finishes its first run and draws single patches."""
  rng = np.random.default_rng(300)
  starts, _ = _interleaved_starts(rng, 5000, 48, 48)
  _check(mosaics, 48, starts, None, 0, ROW_TILES_48)


def test_runs_on_the_production_patch_size(gpu, mosaics):
  """98 patches of 160 x 160 (20 row tiles) through two workgroups with the
  default run length."""
  rng = np.random.default_rng(400)
  starts, _ = _interleaved_starts(rng, 98, 160, 160)
  _check(mosaics, 160, starts, None, 2, 20)
