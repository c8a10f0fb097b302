"""The row band of the lazy / pruned correlation tiles on the device (DESIGN.md
1.3; csrc/sfm_mfma.h: need_tiles, tile_guard; tests/test_guard_band_refs.py is
the arithmetic on the CPU) -- -m gpu.

A finishing tile asks for the rows the peak kernels can read on account of its
hot rows -- the clamped sharpness window of a first peak there and min_distance
rows either side -- instead of 2 x peak_radius rows; a tile is pruned a priori
against the same, narrower band.  Every case compares the default launch with
the kernel that computes and stores every tile (SFM_MFMA_PRUNE=0,
SFM_MFMA_LAZY=0), all four output channels bit for bit, on the smallest geometry
that has the whole mechanism: 64 x 64 patches (a 127-row surface, eight row
tiles, the <4, 5> unit), a few dozen patches, through all, two and four
workgroups (tiles finish in another order; few workgroups carry the need mask
from patch to patch and run the redo phase)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 64
GRIDS = (0, 2, 4)


def _run(pre, post, starts, post_starts=None, patch=P, radius=5, md=2, thr=0.5, mean=None):
  """Reference run (every tile computed and stored), then the default launch
  through all / 2 / 4 workgroups: the same bits.  Returns the reference."""
  from sofima_amd import _abi, flow_field
  starts = np.asarray(starts, np.int32)
  post_starts = starts if post_starts is None else np.asarray(post_starts, np.int32)
  kw = dict(min_distance=md, threshold_rel=thr, peak_radius=radius,
            post_patch_size=(patch, patch), post_starts=post_starts)
  args = (pre, post, None, None, (patch, patch), starts, mean)
  with _abi.option('SFM_MFMA_PRUNE', 0), _abi.option('SFM_MFMA_LAZY', 0):
    ref = np.ascontiguousarray(flow_field.batched_xcorr_peaks(*args, method=2, **kw), np.float32)
  assert ref.shape == (len(starts), 4)
  decoy = _decoy(pre.shape)
  for grid in GRIDS:
    # What a row that is not stored holds is whatever the workspace held before:
    # after the reference run, the right values.  So a launch of the same shape
    # on another image first leaves every surface full of wrong ones -- large, of
    # both signs -- which a max filter or a sharpness window that reads an
    # un-stored row cannot miss.
    with _abi.option('SFM_MFMA_PRUNE', 0), _abi.option('SFM_MFMA_LAZY', 0):
      flow_field.batched_xcorr_peaks(decoy, decoy, *args[2:], method=2, **kw)
    with _abi.option('SFM_MFMA_GRID', grid):
      got = np.ascontiguousarray(flow_field.batched_xcorr_peaks(*args, method=2, **kw), np.float32)
    nan = np.isnan(ref)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=f'grid {grid}')
    same = (got.view(np.uint32) == ref.view(np.uint32)) | nan
    assert same.all(), (f'grid {grid}, R {radius}, md {md}: patches '
                        f'{np.flatnonzero(~same.all(axis=1))[:8]} differ\n'
                        f'{got[~same.all(axis=1)][:4]}\n{ref[~same.all(axis=1)][:4]}')
  return ref


@functools.lru_cache(maxsize=None)
def _decoy(shape):
  """Black-and-white noise: its correlation surfaces are much larger than those
  of the test images, positive and negative."""
  return np.random.default_rng(5).integers(0, 2, shape).astype(np.uint8) * 255


def _grid_starts(h, w, patch=P, step=P // 2):
  ys, xs = np.meshgrid(np.arange(0, h - patch + 1, step), np.arange(0, w - patch + 1, step),
                       indexing='ij')
  return np.stack([ys.ravel(), xs.ravel()], axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _texture(sigma):
  from scipy import ndimage
  rng = np.random.default_rng(2024)
  base = ndimage.gaussian_filter(rng.standard_normal((320 + 2 * 48, 320 + 2 * 48)), sigma)
  base = (base - base.min()) / (base.max() - base.min()) * 255
  base.setflags(write=False)
  return base


def _shifted_pair(dy, dx, sigma=2.0, noise=4.0):
  """320 x 320 EM-like pair, the second image the same content shifted by
  (dy, dx) plus fresh sensor noise."""
  base, m = _texture(sigma), 48
  rng = np.random.default_rng(10000 + 31 * dy + dx)
  pre = base[m:m + 320, m:m + 320]
  post = base[m + dy:m + dy + 320, m + dx:m + dx + 320] + rng.normal(0, noise, (320, 320))
  return (np.clip(np.round(pre), 0, 255).astype(np.uint8),
          np.clip(np.round(post), 0, 255).astype(np.uint8))


def _border_pair(rows, side):
  """Patch pairs whose ONLY common content is a band of `rows` image rows that
  lies at the bottom of the one patch and at the top of the other: the first
  peak sits `rows - 1` rows from the bottom (side 'bottom') or the top of the
  127-row surface, where the sharpness window is pushed back inside the surface.
  (A rigid shift of 60 rows of ordinary texture leaves four rows of overlap, which
  do not carry the maximum; here everything outside the band is flat.)"""
  rng = np.random.default_rng(77 + rows)
  img = (100 + rng.integers(-2, 3, (320, 320))).astype(np.uint8)
  y0 = 160
  img[y0:y0 + rows] = rng.integers(0, 256, (rows, 320))
  post = np.clip(img.astype(np.int32) + rng.integers(-3, 4, img.shape), 0, 255).astype(np.uint8)
  xs = np.arange(8, 320 - P - 8, 8)
  dxs = rng.integers(-3, 4, xs.shape)
  y_low, y_high = y0 + rows - P, y0   # band in the last / in the first rows of the patch
  y_pre, y_post = (y_low, y_high) if side == 'bottom' else (y_high, y_low)
  starts = np.stack([np.full_like(xs, y_pre), xs], axis=1)
  post_starts = np.stack([np.full_like(xs, y_post), xs + dxs], axis=1)
  return img, post, starts, post_starts


def _plateau_pair():
  """Surfaces with a plateau: about the fixed mean 100 the pre patch is one
  bright pixel, so the surface is a shifted copy of the post patch -- zero (cold)
  except for a block of 40 x 64 EQUAL values, every element of which is its own
  window maximum: 2560 candidates for a list of 2048, in three or four of the
  eight row tiles."""
  pre = np.full((320, 320), 100, np.uint8)
  post = np.full((320, 320), 100, np.uint8)
  starts, post_starts = [], []
  for k, (cy, cx) in enumerate([(40, 40), (40, 150), (40, 260), (150, 40), (150, 150),
                                (150, 260), (260, 40), (260, 150), (260, 260)]):
    pre[cy, cx] = 255
    # the bright pixel at another place of every patch, the block at another height
    starts.append((cy - 5 - 6 * k, cx - 8 - 5 * k))
    y_blk = 4 + 2 * k
    post_starts.append((cy - 32, cx - 32))
    post[cy - 32 + y_blk:cy - 32 + y_blk + 40, cx - 32:cx + 32] = 200
  return pre, post, np.array(starts, np.int32), np.array(post_starts, np.int32)


def _list_sizes(pre, post, starts, post_starts, md, thr, mean):
  """(elements above thr x maximum, window maxima among them) of every surface:
  from the CPU oracle, or -- about a fixed integer mean, where ties have to be
  exact as they are in the kernel's integer sums -- from a direct correlation."""
  from scipy import ndimage, signal
  from oracle import flow_oracle
  if mean is None:
    _, surf = flow_oracle.batched_xcorr(pre, post, None, None, (P, P), starts, mean, (P, P),
                                        post_starts, workers=2)
  else:
    cut = lambda img, s: img[s[0]:s[0] + P, s[1]:s[1] + P].astype(np.int64) - int(mean)
    surf = [signal.correlate(cut(pre, a), cut(post, b), 'full', 'direct')
            for a, b in zip(starts, post_starts)]
  out = []
  for s in np.asarray(surf):
    s = s.reshape(s.shape[-2:])
    hot = s > thr * s.max()
    peaks = hot & (s == ndimage.maximum_filter(s, size=2 * md + 1, mode='constant'))
    out.append((int(hot.sum()), int(peaks.sum())))
  return np.array(out)


@pytest.mark.parametrize('dy', range(-9, 10))
def test_peak_at_every_row_offset_of_a_tile(gpu, dy):
  """Rigid shifts of -9 .. +9 rows: the first peak in surface rows 54 .. 72, i.e.
  at every offset inside a 16-row tile and on both sides of the edge between
  tiles 3 and 4, where the band reaches the neighbouring tile or does not."""
  dx = (7 * dy) % 11 - 5
  pre, post = _shifted_pair(dy, dx)
  ref = _run(pre, post, _grid_starts(320, 320))
  assert len(ref) == 81
  # (the case is what it claims: the peak is the content shift)
  assert np.all(np.abs(ref[:, 1]) == abs(dy)) and np.all(np.abs(ref[:, 0]) == abs(dx))


@pytest.mark.parametrize('rows', [1, 2, 3, 5, 6, 7])
@pytest.mark.parametrize('side', ['top', 'bottom'])
def test_first_peak_next_to_the_surface_border(gpu, side, rows):
  """The first peak 0 .. 6 rows from the top / bottom of the surface: within
  peak_radius = 5 rows of it the sharpness window is shifted, not truncated, and
  reads up to 2 x peak_radius rows from the peak; from 5 rows on it is centred.
  With a radius of 8 the shifted window (17 rows) reaches out of the border tile
  (15 rows at the bottom) into its neighbour."""
  pre, post, starts, post_starts = _border_pair(rows, side)
  for radius in (5, 8):
    ref = _run(pre, post, starts, post_starts, radius=radius)
    assert np.all(np.abs(ref[:, 1]) == P - rows), ref[:, 1]
    assert np.all(np.isfinite(ref[:, 2]))


@pytest.mark.parametrize('radius,md', [(1, 1), (5, 2), (8, 2), (2, 7), (30, 2)])
def test_peak_radii_and_min_distances(gpu, radius, md):
  """Window and max filter of every relative size: min_distance above the
  radius (the max-filter rows decide), a window taller than a tile, a radius of
  30 (61 of 127 rows; clamped for the far shifts) -- on peaks at a tile edge,
  inside a tile (five rows from its edge: min_distance = 7 reaches the
  neighbour, a radius of 2 does not), far out and next to the border."""
  for dy, dx, sigma in ((1, -5, 2.0), (-7, 3, 2.0), (5, 2, 2.0), (-5, -3, 2.0),
                        (40, 6, 1.0), (-40, -4, 1.0)):
    pre, post = _shifted_pair(dy, dx, sigma)
    _run(pre, post, _grid_starts(320, 320), radius=radius, md=md)
  for side, rows in (('top', 1), ('bottom', 2), ('top', 4)):
    pre, post, starts, post_starts = _border_pair(rows, side)
    _run(pre, post, starts, post_starts, radius=radius, md=md)


def test_overflowing_hot_and_candidate_lists(gpu):
  """Both fall-backs of the peak kernels sweep stored surfaces with un-stored
  tiles in them (skip mask): a lattice and a broad peak that put more than 4096
  elements above the threshold (hot list), a plateau with more than 2048 window
  maxima (candidate list)."""
  from tests.test_gpu_flow import _prune_images
  starts = _grid_starts(320, 320, step=48)
  for kind in ('fine', 'smooth'):
    pre, post = _prune_images(kind, 31, 320, 320)
    sizes = _list_sizes(pre, post, starts[:4], starts[:4], 1, 0.05, None)
    assert sizes[:, 0].max() > 4096, sizes
    for radius, md in ((5, 1), (5, 2), (2, 7)):
      _run(pre, post, starts, radius=radius, md=md, thr=0.05)
  pre, post, starts, post_starts = _plateau_pair()
  sizes = _list_sizes(pre, post, starts[:1], post_starts[:1], 2, 0.5, 100)
  assert sizes[:, 1].min() > 2048, sizes
  for radius, md in ((5, 2), (8, 2), (2, 7)):
    _run(pre, post, starts, post_starts, radius=radius, md=md, mean=100.0)


def test_first_patches_of_the_bench_geometry(gpu):
  """160 x 160 patches at step 40 (the <10, 11> unit, 20 row tiles): the first
  4 x 4 patches of a 320 x 320 field of the bench's warped pair."""
  import bench
  pre, post = bench.synth_pair(320, 1002, warp=bench.WARP)
  starts = np.stack(np.meshgrid(np.arange(4) * bench.STEP, np.arange(4) * bench.STEP,
                                indexing='ij'), axis=-1).reshape(-1, 2)
  ref = _run(pre, post, starts, patch=bench.PATCH)
  assert np.all(np.isfinite(ref[:, :2]))
