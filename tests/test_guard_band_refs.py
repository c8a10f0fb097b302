"""The row band of the lazy / pruned correlation tiles, restated in NumPy and
checked exhaustively (csrc/sfm_mfma.h: need_tiles, tile_guard).

What the peak kernels read from a stored surface on account of a hot element in
row r (csrc/sfm_xcorr.hip: second_peak_body, is_window_max; reference semantics:
flow_field.py:186-192 and :238-254):

* if it is the first peak, the sharpness window: W = min(2 R + 1, Sy) rows from
  w0(r) = clamp(r - W // 2, 0, Sy - W) -- shifted, not truncated, at the border;
* the max-filter rows r - md .. r + md (clamped addresses).

`need_rows` is what a finishing tile with hot rows [r_lo, r_hi] asks to be
stored, `tile_guard` the rows around a tile that must be cold before the tile
may be left out a priori.  CPU only."""
import numpy as np
import pytest

RADII = (0, 1, 2, 5, 8, 30)
MIN_DISTANCES = (1, 2, 7)
HEIGHTS = range(11, 340)


def _window(r, sy, radius):
  """First and last row of the sharpness window of a first peak in row r."""
  w = min(2 * radius + 1, sy)
  w0 = np.clip(r - w // 2, 0, sy - w)
  return w0, w0 + w - 1


def need_rows(r_lo, r_hi, sy, radius, md):
  """Rows [lo, hi] that must be in memory for hot rows r_lo .. r_hi (need_tiles)."""
  lo = np.maximum(0, np.minimum(_window(r_lo, sy, radius)[0], r_lo - md))
  hi = np.minimum(sy - 1, np.maximum(_window(r_hi, sy, radius)[1], r_hi + md))
  return lo, hi


def tile_guard(p, sy, radius, md):
  """Rows around row tile p that have to be cold for the a-priori skip."""
  w = min(2 * radius + 1, sy)
  t0, t1 = 16 * p, np.minimum(16 * p + 15, sy - 1)
  old = max(md, 2 * radius)
  return np.where((t0 <= w - 1) | (t1 >= sy - w), old, max(md, w // 2))


def _read_rows(r, sy, radius, md):
  """Lowest and highest row read for a first peak in row r."""
  w0, w1 = _window(r, sy, radius)
  return np.minimum(w0, np.maximum(r - md, 0)), np.maximum(w1, np.minimum(r + md, sy - 1))


@pytest.mark.parametrize('md', MIN_DISTANCES)
@pytest.mark.parametrize('radius', RADII)
def test_requested_rows_hold_every_row_the_peak_kernels_read(radius, md):
  """Every row of [w0(r), w0(r) + W - 1] and of [r - md, r + md] lies in the
  extents requested by a tile whose hot rows include r -- for every first and
  last hot row the tile may have -- and the extents stay inside today's
  `guard` rows (max(md, 2 R)) around the hot rows."""
  guard = max(md, 2 * radius)
  cases = 0
  for sy in HEIGHTS:
    r = np.arange(sy)
    rd_lo, rd_hi = _read_rows(r, sy, radius, md)
    lo1, hi1 = need_rows(r, r, sy, radius, md)
    assert np.all(lo1 <= rd_lo) and np.all(hi1 >= rd_hi)
    # never more than today's band
    assert np.all(lo1 >= np.maximum(r - guard, 0)) and np.all(hi1 <= np.minimum(r + guard, sy - 1))
    # every pair of hot rows r_lo <= r <= r_hi inside one tile
    for t0 in range(0, sy, 16):
      rows = np.arange(t0, min(t0 + 16, sy))
      r_lo, r_hi, k = np.meshgrid(rows, rows, rows, indexing='ij')
      inside = (r_lo <= k) & (k <= r_hi)     # k: any hot row between them
      lo, hi = need_rows(r_lo, r_hi, sy, radius, md)
      assert np.all(lo[inside] <= rd_lo[k[inside]]) and np.all(hi[inside] >= rd_hi[k[inside]])
      cases += int(inside.sum())
  assert cases > 100000


@pytest.mark.parametrize('md', MIN_DISTANCES)
@pytest.mark.parametrize('radius', RADII)
def test_no_tile_is_read_from_beyond_its_guard(radius, md):
  """A tile is left out a priori when every element within tile_guard rows of it
  is cold.  So for every peak row r, every tile touched by the window or the
  max-filter rows of r lies within its own guard of r; and no guard exceeds
  today's."""
  guard = max(md, 2 * radius)
  for sy in HEIGHTS:
    n_tiles = (sy + 15) // 16
    p = np.arange(n_tiles)
    g = tile_guard(p, sy, radius, md)
    assert np.all(g <= guard) and np.all(g >= md)
    t0, t1 = 16 * p, np.minimum(16 * p + 15, sy - 1)
    r = np.arange(sy)[:, None]
    rd_lo, rd_hi = _read_rows(r, sy, radius, md)
    touched = (rd_lo <= t1[None, :]) & (rd_hi >= t0[None, :])
    dist = np.maximum(0, np.maximum(t0[None, :] - r, r - t1[None, :]))
    assert np.all(dist[touched] <= np.broadcast_to(g, dist.shape)[touched]), (sy, radius, md)


def test_defaults_and_a_window_taller_than_the_surface():
  """Sy = 319, R = 5, md = 2: five rows either side away from the border, the
  shifted window next to it; 2 R + 1 > Sy asks for the whole surface."""
  assert need_rows(100, 103, 319, 5, 2) == (95, 108)
  assert need_rows(2, 2, 319, 5, 2) == (0, 10)
  assert need_rows(317, 318, 319, 5, 2) == (308, 318)
  assert need_rows(40, 40, 319, 1, 7) == (33, 47)
  assert need_rows(7, 9, 21, 30, 2) == (0, 20)
  assert list(tile_guard(np.arange(20), 319, 5, 2)) == [10] + [5] * 18 + [10]
  assert list(tile_guard(np.arange(2), 21, 30, 2)) == [60, 60]
