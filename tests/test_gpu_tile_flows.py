"""The montage fine-flow stage on the GPU (-m gpu): `filter_flow_maps` (one
launch for a ragged batch of tile pairs), `aggregate_arrays(device_output=True)`
and `compute_flow_map(device_output=True)`, bit for bit (NaNs equal) against the
reference's golden output and the restatement of tests/tile_flows_ref.py."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import tile_flows_ref as ref
from tests.test_gpu_reconcile import _snake, _spiral
from tests.util import em_texture

pytestmark = pytest.mark.gpu

CLEAN = dict(min_peak_ratio=1.0, min_peak_sharpness=1.5, max_magnitude=14.0, max_deviation=5.0)
RECONCILE = dict(max_gradient=6.0, max_deviation=4.0, min_patch_size=3)


def _same(got, want, what=''):
  got = np.asarray(got)
  assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
  if not np.array_equal(got, want, equal_nan=True):
    diff = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    idx = np.argwhere(diff)[:5]
    raise AssertionError(f'{what}: {int(diff.sum())} elements differ, first at {idx.tolist()}: '
                         f'got {[got[tuple(i)] for i in idx]}, want {[want[tuple(i)] for i in idx]}')


def _check(tf, flows, clean, reconcile, what=''):
  """A TileFlows against the restatement: every pair, the padding of `data`."""
  assert list(tf) == list(flows) and len(tf) == len(flows)
  host = tf.to_host()
  data = np.asarray(tf.data)
  assert data.dtype == np.float32 and data.shape[:2] == (2, len(flows))
  if flows:
    assert data.shape[2:] == tuple(np.max([v.shape[1:] for v in flows.values()], axis=0))
  for i, (k, v) in enumerate(flows.items()):
    want = ref.filter_pair(np.asarray(v), clean, reconcile)
    _same(host[k], want, f'{what} {k}')
    h, w = want.shape[1:]
    assert tuple(tf.shapes[i]) == (h, w) and tf[k].shape == (2, h, w)
    pad = data[:, i].copy()
    pad[:, :h, :w] = np.nan
    assert np.isnan(pad).all(), f'{what} {k}: values outside the extent'
  return host


def _pair(rng, c, h, w, holes=0.3):
  """Smoothed-noise vectors with outliers, sharpness, ratio, blobs of NaN."""
  f = np.stack([ndimage.gaussian_filter(rng.standard_normal((h, w)), 1.5) * 12
                for _ in range(2)]).astype(np.float32)
  hit = rng.random((h, w)) < 0.08
  f[:, hit] += rng.uniform(-20, 20, (2, int(hit.sum()))).astype(np.float32)
  if c == 4:
    f = np.concatenate([f, rng.uniform(-6, 6, (1, h, w)).astype(np.float32),
                        rng.choice([0, 0.2, 0.6, 1.5, 3.0], (1, h, w)).astype(np.float32)])
  if holes:
    noise = ndimage.gaussian_filter(rng.standard_normal((h, w)), 1.0)
    f[:, noise > np.quantile(noise, 1 - holes)] = np.nan
  if h * w > 6:
    f[int(rng.integers(0, 2)), int(rng.integers(0, h)), int(rng.integers(0, w))] = np.nan
  return f


def test_golden_filter_and_aggregate(gpu, golden):
  from sofima_amd import _dev, stitch_elastic
  g = golden('tile_flows')
  n = 0
  for mname, d, pname, flows, clean, rec, want in ref.filter_cases(g):
    tf = stitch_elastic.filter_flow_maps(flows, clean, rec)
    assert isinstance(tf, stitch_elastic.TileFlows) and tf.batched.all()
    host = tf.to_host()
    assert list(host) == list(want)
    for k in want:
      _same(host[k], want[k], f'{mname} {d} {pname} {k}')
    n += len(want)
  assert n >= 150
  psets = ref.parameter_sets(g)
  for name in g['montages']:
    m = ref.montage(g, name)
    out = stitch_elastic.aggregate_arrays(*ref.aggregate_args(m), device_output=True)
    for got, want in zip(out[:3], m['want'][:3]):
      assert isinstance(got, _dev.DeviceArray) and got.dtype == np.float32
      _same(got, want.astype(np.float32), f'{name} device')
    _same(out[3], m['want'][3], f'{name} nbors')
    assert out[4] == m['want_idx']
    if len(m['stride']) != 2:
      continue
    # the filtered flows, as a TileFlows, as DeviceArrays and as host arrays
    clean, rec = psets['all']
    tfs = {d: stitch_elastic.filter_flow_maps(m[d], clean, rec) for d in 'xy'}
    hosts = {d: tfs[d].to_host() for d in 'xy'}
    want = ref.aggregate_arrays(*ref.aggregate_args(m, hosts['x'], hosts['y']))
    for fine in (tfs, {d: dict(tfs[d].items()) for d in 'xy'}, hosts):
      for dev_out in (True, False):
        got = stitch_elastic.aggregate_arrays(*ref.aggregate_args(m, fine['x'], fine['y']),
                                              device_output=dev_out)
        for a, b in zip(got[:3], want[:3]):
          _same(a, b.astype(np.float32) if dev_out else b, f'{name} filtered {dev_out}')
        _same(got[3], want[3])


def test_ragged_fuzz(gpu):
  from sofima_amd import stitch_elastic
  rng = np.random.default_rng(77)
  f32_edge = [0, 0.1, 1.1, 0.7, 2.0, 5.0, 14.0]
  for it in range(40):
    n = int(rng.integers(1, 13))
    flows = {(i, it): _pair(rng, int(rng.choice([2, 4])), int(rng.integers(1, 41)),
                            int(rng.integers(1, 41)), float(rng.uniform(0.1, 0.6)))
             for i in range(n)}
    num = np.float64 if it % 3 == 2 else float    # float64 scalars compare in double
    clean = dict(min_peak_ratio=num(rng.choice([0, 0.6, 1.1, 1.5])),
                 min_peak_sharpness=num(rng.choice([0, 0.7, 1.1, 3.3])),
                 max_magnitude=num(rng.choice(f32_edge + [-1.0])),
                 max_deviation=num(rng.choice(f32_edge)))
    rec = dict(max_gradient=num(rng.choice(f32_edge + [3.3, 9.0])),
               max_deviation=num(rng.choice(f32_edge)),
               min_patch_size=int(rng.choice([0, 1, 2, 3, 7, 20, 150])))
    if it % 5 == 3:
      clean = None
    if it % 7 == 5:
      rec = None
    tf = stitch_elastic.filter_flow_maps(flows, clean, rec)
    assert tf.batched.all()
    _check(tf, flows, clean, rec, f'batch {it} {clean} {rec}')


def test_smallest_extents(gpu):
  from sofima_amd import stitch_elastic
  rng = np.random.default_rng(3)
  flows = {(i, 0): _pair(rng, 4, h, w, 0) for i, (h, w) in
           enumerate([(1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (40, 40)])}
  flows[0, 1] = np.full((4, 5, 6), np.nan, np.float32)            # all NaN
  full = _pair(rng, 2, 9, 8, 0)
  full[np.isnan(full)] = 1
  flows[1, 1] = full                                              # no NaN
  quirk = np.ones((2, 6, 5), np.float32)
  quirk[0, 2, 3] = np.nan                                         # n0 = 1 < 3
  flows[2, 1] = quirk
  inf = _pair(rng, 4, 8, 9)
  inf[0, 1, 1], inf[1, 5, 5], inf[2, 0, 0], inf[3, 7, 7] = np.inf, -np.inf, np.inf, -np.inf
  flows[3, 1] = inf
  for clean, rec in ((CLEAN, RECONCILE), (None, RECONCILE), (CLEAN, None),
                     (None, dict(max_gradient=0, max_deviation=0, min_patch_size=3))):
    host = _check(stitch_elastic.filter_flow_maps(flows, clean, rec), flows, clean, rec)
  assert np.isnan(host[2, 1][:, 2, 3]).all() and np.isnan(host[2, 1]).sum() == 2


def test_more_workgroups_than_cus(gpu):
  from sofima_amd import stitch_elastic
  rng = np.random.default_rng(600)
  flows = {(i % 30, i // 30): _pair(rng, 4 if i % 3 else 2, int(rng.integers(3, 7)),
                                    int(rng.integers(3, 7)), 0.2) for i in range(600)}
  tf = stitch_elastic.filter_flow_maps(flows, CLEAN, dict(RECONCILE, min_patch_size=2))
  assert tf.batched.all() and tf.data.shape == (2, 600, 6, 6)
  _check(tf, flows, CLEAN, dict(RECONCILE, min_patch_size=2))


def test_long_chains_in_lds(gpu):
  """A spiral and a snake in one (64, 96) pair: the longest chains the union-find
  in LDS meets, next to tiny pairs."""
  from sofima_amd import stitch_elastic
  valid = np.zeros((64, 96), bool)
  valid[:, :46] = _spiral(64, 46)
  valid[:, 48:] = _snake(64, 48)
  lab, n = ndimage.label(valid)
  sizes = np.sort(np.bincount(lab.ravel())[1:])
  assert n == 2 and sizes[0] > 700 and sizes[0] != sizes[1], sizes
  f = np.where(valid, 1.0, np.nan).astype(np.float32)[None].repeat(2, 0)
  rng = np.random.default_rng(8)
  flows = {(0, 0): _pair(rng, 2, 3, 4), (1, 0): f, (2, 0): _pair(rng, 2, 2, 2, 0)}
  kept = []
  for patch in (int(sizes[0]) - 1, int(sizes[0]) + 1, int(sizes[1]) - 1, int(sizes[1]) + 1):
    rec = dict(max_gradient=0, max_deviation=0, min_patch_size=patch)
    tf = stitch_elastic.filter_flow_maps(flows, None, rec)
    assert tf.batched.all()
    kept.append(int((~np.isnan(_check(tf, flows, None, rec, f'min {patch}')[1, 0][0])).sum()))
  assert kept == [int(sizes.sum()), int(sizes[1]), int(sizes[1]), 0]


def test_the_cap(gpu):
  from sofima_amd import _abi, stitch_elastic
  cap = _abi.load().sfm_filter_tile_flows_max_nodes()
  rng = np.random.default_rng(13)
  flows = {(0, 0): _pair(rng, 4, 5, 4), (1, 0): _pair(rng, 4, cap // 64, 64),
           (2, 0): _pair(rng, 2, 3, 3, 0), (3, 0): _pair(rng, 4, cap // 64 + 1, 64),
           (4, 0): _pair(rng, 2, 6, 2)}
  assert flows[1, 0].shape[1] * 64 == cap
  for clean, rec in ((CLEAN, dict(RECONCILE, min_patch_size=40)), (None, RECONCILE)):
    tf = stitch_elastic.filter_flow_maps(flows, clean, rec)
    assert tf.batched.tolist() == [True, True, True, False, True]
    _check(tf, flows, clean, rec, 'cap')


def test_input_handling(gpu):
  from sofima_amd import _dev, stitch_elastic
  rng = np.random.default_rng(21)
  host = {(i, 0): _pair(rng, 4 if i % 2 else 2, 5 + i, 9 - i) for i in range(6)}
  host[6, 0] = host[0, 0].astype(np.float64)
  keep = {k: v.copy() for k, v in host.items()}
  mixed, clones = {}, {}
  for i, (k, v) in enumerate(host.items()):
    if i % 3 == 0:
      mixed[k] = v
    elif i % 3 == 1:
      mixed[k] = torch.from_numpy(v.copy()).to(gpu)
      clones[k] = mixed[k].clone()
    else:
      mixed[k] = _dev.DeviceArray(torch.from_numpy(v.copy()).to(gpu))
      clones[k] = mixed[k].tensor.clone()
  on_device = {k: _dev.DeviceArray(torch.from_numpy(np.asarray(v, np.float32)).to(gpu))
               for k, v in host.items()}
  first = _check(stitch_elastic.filter_flow_maps(host, CLEAN, RECONCILE), host, CLEAN, RECONCILE)
  for flows in (mixed, on_device, host):
    again = stitch_elastic.filter_flow_maps(flows, CLEAN, RECONCILE).to_host()
    for k in first:
      _same(again[k], first[k], f'{k}')
  for k, v in host.items():
    assert np.array_equal(v, keep[k], equal_nan=True) and v.dtype == keep[k].dtype
  for k, c in clones.items():
    t = mixed[k].tensor if isinstance(mixed[k], _dev.DeviceArray) else mixed[k]
    assert torch.equal(t.view(torch.int32), c.view(torch.int32))   # the bits
  empty = stitch_elastic.filter_flow_maps({}, CLEAN, RECONCILE)
  assert len(empty) == 0 and empty.to_host() == {} and empty.data.shape[:2] == (2, 0)
  with pytest.raises(ValueError):
    stitch_elastic.filter_flow_maps({(0, 0): np.zeros((3, 4, 4), np.float32)}, CLEAN, None)
  with pytest.raises(KeyError):
    first_tf = stitch_elastic.filter_flow_maps(host, None, None)
    first_tf[9, 9]


@pytest.fixture(scope='module')
def montage2x2():
  """2 x 2 tiles of 256^2 cut from one texture, 64 px overlaps, each tile a few
  pixels off its nominal place so that the fine flows are not zero."""
  rng = np.random.default_rng(42)
  base = em_texture(rng, (256 + 192 + 16, 256 + 192 + 16))
  tiles = {}
  for (x, y), (jx, jy) in zip(((0, 0), (1, 0), (0, 1), (1, 1)), ((0, 0), (3, -2), (-2, 2), (2, 3))):
    y0, x0 = 8 + 192 * y + jy, 8 + 192 * x + jx
    tiles[x, y] = base[y0:y0 + 256, x0:x0 + 256].copy()
  cx = np.full((2, 2, 2), np.nan)
  cy = np.full((2, 2, 2), np.nan)
  cx[:, :, 0] = np.array([-64.0, 0.0])[:, None]
  cy[:, 0, :] = np.array([0.0, -64.0])[:, None]
  return tiles, cx, cy


def _flow_maps(montage, device_output):
  from sofima_amd import stitch_elastic
  tiles, cx, cy = montage
  kw = dict(patch_size=(32, 32), stride=(16, 16), batch_size=64)
  return (stitch_elastic.compute_flow_map(tiles, cx, 0, device_output=device_output, **kw),
          stitch_elastic.compute_flow_map(tiles, cy, 1, device_output=device_output, **kw))


def test_compute_flow_map_device_output(gpu, montage2x2):
  from sofima_amd import _dev
  (hx, hox), (hy, hoy) = _flow_maps(montage2x2, False)
  (dx, dox), (dy, doy) = _flow_maps(montage2x2, True)
  assert hox == dox and hoy == doy and list(hx) == list(dx) and list(hy) == list(dy)
  assert len(hx) == 2 and len(hy) == 2
  for h, d in ((hx, dx), (hy, dy)):
    for k in h:
      assert isinstance(d[k], _dev.DeviceArray)
      _same(d[k], h[k], f'flow {k}')
      assert np.isnan(h[k][:, 0]).all() and np.isfinite(h[k][:2, 1:, 1:]).any()


def test_end_to_end_montage(gpu, montage2x2):
  """correlation peaks -> filters -> packing -> mesh solve without leaving the
  device == the same chain through host dicts and one call per tile pair."""
  from sofima_amd import flow_utils, mesh, stitch_elastic
  tiles, cx, cy = montage2x2
  clean = dict(min_peak_ratio=1.4, min_peak_sharpness=1.4, max_magnitude=80, max_deviation=5)
  rec = dict(max_gradient=-1, max_deviation=5, min_patch_size=4)
  coords = [(0, 0), (1, 0), (0, 1), (1, 1)]
  coarse = np.zeros((2, 2, 2))
  stride, tile_shape = (16, 16), (256, 256)
  cfg = mesh.IntegrationConfig(dt=0.001, gamma=0.0, k0=0.01, k=0.1, stride=stride,
                               num_iters=100, max_iters=100, stop_v_max=1e-9, dt_max=100,
                               prefer_orig_order=True, start_cap=0.1, final_cap=10.0,
                               remove_drift=True)

  def solve(fx, fy, x, nbors):
    fn = stitch_elastic.TargetMeshFn(nbors, fx, fy, stride)
    return np.asarray(mesh.relax_mesh(x, None, cfg, prev_fn=fn)[0])

  (dx, ox), (dy, oy) = _flow_maps(montage2x2, True)
  fine_x = stitch_elastic.filter_flow_maps(dx, clean, rec)
  fine_y = stitch_elastic.filter_flow_maps(dy, clean, rec)
  fx, fy, x, nbors, idx = stitch_elastic.aggregate_arrays(
      (cx, fine_x, ox), (cy, fine_y, oy), coords, coarse, stride, tile_shape,
      device_output=True)
  got = solve(fx, fy, x, nbors)

  (hx, ox2), (hy, oy2) = _flow_maps(montage2x2, False)
  per_pair = []
  for flows in (hx, hy):
    per_pair.append({k: np.asarray(flow_utils.reconcile_flows(
        [flow_utils.clean_flow(v[:, None], **clean)], **rec))[:, 0] for k, v in flows.items()})
  hfx, hfy, hxx, hnb, hidx = stitch_elastic.aggregate_arrays(
      (cx, per_pair[0], ox2), (cy, per_pair[1], oy2), coords, coarse, stride, tile_shape)
  assert hfx.dtype == np.float64 and idx == hidx
  _same(nbors, hnb)
  _same(fx, hfx.astype(np.float32), 'fx')
  _same(fy, hfy.astype(np.float32), 'fy')
  assert np.isfinite(hfx).any() and np.isfinite(hfy).any()
  want = solve(hfx, hfy, hxx, hnb)
  _same(got, want, 'relaxed mesh')
  assert np.isfinite(want).all() and np.abs(want).max() > 0
