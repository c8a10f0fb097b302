"""Edge tests of the montage kernels (-m gpu): the target mesh
(`target_mesh_kernel` / sfm_target.h, alone and as the `prev_fn` of a tiled
relaxation), the tile-mesh force and the dynamic-range mask, at the shapes,
special values and limits where kernels go wrong.

Every kernel is pinned twice: to its float32 oracle, bit for bit (the kernels
follow the oracles' operation order), and to an independent float64
restatement written from the definition, under a bound derived from the
roundings involved.  The case builders and the float64 references live at
module level and need no GPU: tests/test_montage_refs.py asserts the reference
side (the float32 oracle stays inside the derived bounds, the cases cover what
they claim, the limit forms are not vacuous) on the CPU over the SAME cases.

Out of contract, not tested: a recorded flow size (`flow_size_ortho`,
`flow_size_overlap`, `flow_size_z`) larger than the tile mesh makes the paste
origin negative; the reference's dynamic slices clamp there, neither the oracle
nor the kernel does.  Neighbour or flow indices outside the tile / flow arrays
are out of contract as well.  No test passes such input.

NaN pixels are left out of the range-mask tests: SciPy's rank filters answer
differently for an image and its mirror image once a window holds a NaN (the
result hangs on the scan order, not on the window's contents alone;
test_montage_refs.py shows it), so there is no reference to pin.
"""
import numpy as np
import pytest

from oracle import maps_oracle, mesh_oracle, stitch_oracle
from tests.refs64 import around, compose64, compose_atol, smooth

pytestmark = pytest.mark.gpu
f32 = np.float32
FLT_MAX = float(np.finfo(f32).max)


def _frozen(*arrays):
  for a in arrays:
    a.setflags(write=False)
  return arrays


# ---------------------------------------------------------------------------
# Target mesh: cases
# ---------------------------------------------------------------------------
def montage_case(seed, gx, gy, mesh_shape, overlap, stride, pads=((1, 3), (4, 2)), amp=4.0,
                 offs=(-2, 0, 3), offs_z=(0,), zero_flow=False, drop_pairs=(), holes=0.02):
  """gx x gy tiles of `mesh_shape` ((y, x) or (z, y, x)) nodes with flow strips
  `overlap` nodes wide between adjacent tiles, laid out like the reference's
  aggregated arrays (stitch_elastic.py:285-453):

  * neighbour rows in the fixed slots left, right, up, down, -1 where there is
    no neighbour (so -1 rows precede valid ones);
  * per pair a recorded flow size: `overlap` along the connection, the mesh
    size minus |coarse_offset_ortho| across it (the whole axis where the offset
    is 0), one node less than the mesh in z where the mesh has several;
  * the flow arrays padded with NaN beyond the recorded sizes to a common shape
    plus `pads` = ((y, x) for fx, (y, x) for fy) more nodes (1 / 2 in z), so fx
    and fy differ in shape, and n_fx != n_fy (fy has one unused entry more; the
    entries no pair owns hold finite junk);
  * coarse_offset_ortho / coarse_offset_z cycle through `offs` / `offs_z` over
    the pairs; every pair yields a mult = +1 row (in the second tile) and a
    mult = -1 row (in the first).

  drop_pairs: ('x' | 'y', first tile) pairs that get no rows at all.
  Returns dict(nbors, fx, fy, x, stride)."""
  rng = np.random.default_rng(seed)
  nd = len(mesh_shape)
  n = gx * gy
  my, mx = mesh_shape[-2:]
  mz = mesh_shape[0] if nd == 3 else 1
  f_z = max(1, mz - 1)
  fields = 8 if nd == 2 else 11

  pairs = {'x': [t for t in range(n) if t % gx < gx - 1 and ('x', t) not in drop_pairs],
           'y': [t for t in range(n) if t // gx < gy - 1 and ('y', t) not in drop_pairs]}
  info = {}
  k = 0
  for kind in 'xy':
    for t in pairs[kind]:
      off_o = offs[k % len(offs)]
      off_z = offs_z[(k // len(offs) + k) % len(offs_z)]
      k += 1
      ortho_n = my if kind == 'x' else mx
      info[kind, t] = dict(off_o=off_o, off_z=off_z, f_ortho=max(1, ortho_n - abs(off_o)),
                           fine=rng.integers(-2, 3, 3))

  def flows(kind, count, pad, pad_z):
    sizes = [(i['f_ortho'], overlap) if kind == 'x' else (overlap, i['f_ortho'])
             for (kk, _), i in info.items() if kk == kind] or [(1, 1)]
    shape = (max(s[0] for s in sizes) + pad[0], max(s[1] for s in sizes) + pad[1])
    lead = (f_z + pad_z,) if nd == 3 else ()
    arr = np.full((nd, count) + lead + shape, np.nan, f32)
    for t in range(count):
      if (kind, t) not in info:     # owned by no pair: must never be read as data
        arr[:, t] = rng.uniform(-50, 50, arr[:, t].shape)
        continue
      i = info[kind, t]
      real = (f_z,) * (nd - 2) + ((i['f_ortho'], overlap) if kind == 'x' else
                                  (overlap, i['f_ortho']))
      data = np.stack([smooth(rng, real, 0.0 if zero_flow else amp) for _ in range(nd)])
      if holes and not zero_flow:
        data[:, rng.random(real) < holes] = np.nan
      arr[(slice(None), t) + tuple(slice(0, s) for s in real)] = data
    return arr

  fx = flows('x', n, pads[0], 1)
  fy = flows('y', n + 1, pads[1], 2)
  x = np.stack([np.stack([smooth(rng, tuple(mesh_shape), amp / 2) for _ in range(n)])
                for _ in range(nd)]).astype(f32)

  nb = -np.ones((n, 4, fields), np.int32)

  def row(nbor, kind, first):
    i = info[kind, first]
    e = -np.ones(fields, np.int32)
    e[0], e[1], e[2], e[3], e[4] = nbor, first, i['off_o'], i['f_ortho'], overlap
    e[5], e[6], e[7] = i['fine'][0], i['fine'][1], 0 if kind == 'x' else 1
    if nd == 3:
      e[8], e[9], e[10] = i['off_z'], f_z, i['fine'][2]
    return e

  for t in range(n):
    if ('x', t - 1) in info and t % gx > 0:
      nb[t, 0] = row(t - 1, 'x', t - 1)        # nbor == flow_idx: mult = +1
    if ('x', t) in info:
      nb[t, 1] = row(t + 1, 'x', t)            # mult = -1
    if ('y', t - gx) in info:
      nb[t, 2] = row(t - gx, 'y', t - gx)
    if ('y', t) in info:
      nb[t, 3] = row(t + gx, 'y', t)
  return dict(nbors=nb, fx=fx, fy=fy, x=x, stride=tuple(float(s) for s in stride))


def _corner_flow_nans(case, overlap):
  """NaN in ONE flow component, and in both, inside the corner of tile 0 where
  its x strip (right neighbour) and its y strip (lower neighbour, pasted later)
  overlap: the lower right `overlap` x `overlap` nodes.  Both rows of tile 0 have
  mult = -1, so the corner is the last `overlap` columns of fy[:, 0]'s recorded
  part and the last `overlap` rows of fx[:, 0]'s."""
  nb = case['nbors']
  f_ortho_y = int(nb[0, 3, 3])       # recorded x size of the y pair's flow
  f_ortho_x = int(nb[0, 1, 3])
  fy, fx = case['fy'], case['fx']
  c0 = f_ortho_y - overlap
  fy[:, 0, :overlap, c0:f_ortho_y] = np.nan_to_num(fy[:, 0, :overlap, c0:f_ortho_y])
  fy[0, 0, 1, c0 + 1] = np.nan          # x component only
  fy[1, 0, 2, c0 + 2] = np.nan          # y component only
  fy[:, 0, 3, c0 + 3] = np.nan          # both
  fy[0, 0, 0, c0:f_ortho_y] = np.nan    # a whole corner row, x component
  r0 = f_ortho_x - overlap
  fx[:, 0, r0:f_ortho_x, :overlap] = np.nan_to_num(fx[:, 0, r0:f_ortho_x, :overlap])
  fx[1, 0, r0 + 2, 1] = np.nan          # the earlier update NaN, the later one valid
  fx[:, 0, r0 + 3, 3] = np.nan          # NaN in both updates: the node stays NaN


_CASES = {}


def target_cases():
  """{name: case}; built once, read-only."""
  if _CASES:
    return _CASES
  c = {}
  # block-edge geometries: with 5 .. 7 node strips the paste regions end one
  # short of, on and one past a 16-node block edge; three strides
  c['g22_15x31'] = montage_case(1, 2, 2, (15, 31), 5, (20, 20), offs=(-2, 3, 0))
  c['g22_16x16'] = montage_case(2, 2, 2, (16, 16), 6, (16, 10.5), pads=((2, 1), (3, 4)),
                                offs=(0, -2, 3))
  c['g22_17x33'] = montage_case(3, 2, 2, (17, 33), 7, (20, 20), pads=((4, 2), (1, 3)),
                                offs=(3, 0, -2, 0))
  # one row / one column of tiles; strips that cover a whole axis
  c['g31_5x40'] = montage_case(4, 3, 1, (5, 40), 6, (16, 10.5), offs=(0, -1))
  c['g13_40x5'] = montage_case(5, 1, 3, (40, 5), 6, (20, 20), offs=(1, 0))
  c['g13_5x40'] = montage_case(6, 1, 3, (5, 40), 5, (20, 20), offs=(-3, 2))   # overlap = all of y
  c['g31_40x5'] = montage_case(7, 3, 1, (40, 5), 5, (16, 10.5), offs=(2, -3))  # overlap = all of x
  # wide enough (x >= 40, y >= 4) for the tiled integrator: the prev_fn tests
  c['g22_15x47'] = montage_case(8, 2, 2, (15, 47), 5, (20, 20), offs=(-2, 3, 0))
  c['g22_16x48'] = montage_case(9, 2, 2, (16, 48), 6, (16, 10.5), offs=(3, 0, -2))
  c['g22_17x49_nan'] = montage_case(10, 2, 2, (17, 49), 7, (20, 20), offs=(0, -2, 0, 3),
                                    holes=0.0)
  _corner_flow_nans(c['g22_17x49_nan'], 7)
  c['g22_17x33_nan'] = montage_case(11, 2, 2, (17, 33), 6, (16, 10.5), offs=(0, 3, 0, -2),
                                    holes=0.0)
  _corner_flow_nans(c['g22_17x33_nan'], 6)
  # tile 2 has no pair: four -1 rows, all-NaN output
  c['isolated_tile'] = montage_case(12, 3, 1, (16, 16), 5, (20, 20), drop_pairs=(('x', 1),))
  # queries leave the neighbour mesh on every side
  c['large_amp'] = montage_case(13, 2, 2, (16, 16), 6, (20, 20), amp=70.0, offs=(0, 0, -2, 3))
  # zero flow: every query ON a node; the mult = +1 strips reach the last node,
  # whose upper corner is out of range with weight 0 and still gives NaN
  c['zero_flow'] = montage_case(14, 2, 2, (15, 31), 5, (16, 10.5), zero_flow=True,
                                offs=(0, -2, 3))
  # NaN / inf nodes in x: single components, near the corners the strips sample
  case = montage_case(15, 2, 2, (17, 33), 7, (20, 20), offs=(0, 0, 0, 0), holes=0.0)
  x = case['x']
  for t in range(4):
    x[0, t, 2, 3] = np.nan          # sampled by mult = -1 rows (top / left strips)
    x[1, t, 3, 29] = np.nan
    x[0, t, 14, 29] = np.nan        # sampled by mult = +1 rows (bottom / right strips)
    x[1, t, 13, 4] = np.nan
    x[:, t, 15, 15] = np.nan
    x[0, t, 1, 16] = np.inf
    x[1, t, 15, 2] = -np.inf
    x[0, t, 8, 30] = -np.inf
    x[0, t, 8, 31] = np.inf         # inf - inf between neighbours
  c['nonfinite_x'] = case
  # volumetric
  for name, (gx, gy) in (('21', (2, 1)), ('12', (1, 2))):
    for tag, oz in (('zneg', -1), ('z0', 0), ('zpos', 2)):
      c[f'vol{name}_{tag}'] = montage_case(
          20 + len(c), gx, gy, (4, 9, 18), 5, (8, 16, 20), offs=(2, -1, 0)[len(c) % 3:] + (0,),
          offs_z=(oz,), pads=((1, 2), (3, 1)))
    # one section: node 0 is also the LAST node in z, its upper corner is always
    # out of range, so every update is NaN in the reference itself
    c[f'vol{name}_thin'] = montage_case(30 + len(c), gx, gy, (1, 6, 17), 5, (8, 16, 20),
                                        offs=(-1,) if gx == 2 else (2,), pads=((2, 1), (1, 2)))
  for case in c.values():
    _frozen(case['nbors'], case['fx'], case['fy'], case['x'])
  _CASES.update(c)
  return _CASES


PREV_FN_CASES = ('g22_15x47', 'g22_16x48', 'g22_17x49_nan', 'g31_5x40')
SINGLE_TILE_CASES = ('g22_17x33', 'g31_5x40', 'isolated_tile', 'vol21_zneg')


# ---------------------------------------------------------------------------
# Target mesh: float64 reference
# ---------------------------------------------------------------------------
def target64(nbors, x, fx, fy, stride, stats=None):
  """compute_target_mesh for every tile from the definition
  (stitch_elastic.py:456-676), in double.  Per neighbour row, in order:
  compose64(mult * flow @ start, neighbour mesh @ 0, 'constant'), add
  mult * fine offsets, paste at the target origin into a NaN canvas extended
  by the flow array size, a NaN update keeping the previous value per
  component; crop to the mesh.

  Returns (result, near, M): `near` marks nodes that received an update from a
  query within 4 float32 ulps of a node index without being on it (see
  compose64); M is the largest finite absolute coordinate met: sampled
  positions |ref + x| of the neighbour meshes and |update|.

  stats: a dict that receives what the cases claim to cover -- 'cropped'
  (pastes that run past the mesh), 'survive_one' (nodes where an earlier
  update survives in some but not all components while the later one sets
  the others), 'out' ({(axis, 'lo' | 'hi')} of queries outside the neighbour
  mesh), 'last' (queries exactly on the last node of an axis), 'signs'
  ({(sign coarse_offset_ortho, mult, dim)}), 'signs_z', 'all_nan_tiles',
  'minus_before_valid'."""
  x = np.asarray(x, f32)
  nd = x.shape[0]
  msz = x.shape[2:]
  st = tuple(float(s) for s in stride)
  assert len(st) == nd
  out = np.full(x.shape, np.nan)
  near = np.zeros(x.shape[1:], bool)
  big = 0.0
  if stats is not None:
    stats.update(cropped=0, survive_one=0, out=set(), last=0, signs=set(), signs_z=set(),
                 all_nan_tiles=0, minus_before_valid=0)
  ext = [msz[i] + max(fx.shape[2 + i], fy.shape[2 + i]) for i in range(nd)]
  crop = tuple(slice(0, s) for s in msz)
  y_ax, x_ax = nd - 2, nd - 1
  for t, rows in enumerate(np.asarray(nbors)):
    canvas = np.full([nd] + ext, np.nan)
    cnear = np.zeros(ext, bool)
    seen_minus = False
    for nb in rows:
      nbor, flow_idx, off_o, f_o, f_ov, fine_x, fine_y, dim = (int(v) for v in nb[:8])
      if nbor == -1:
        seen_minus = True
        continue
      if stats is not None and seen_minus:
        stats['minus_before_valid'] += 1
      mult = 1 if nbor == flow_idx else -1
      flow = fx if dim == 0 else fy
      par, ortho = (x_ax, y_ax) if dim == 0 else (y_ax, x_ax)
      start, tg = [0] * nd, [0] * nd
      start[par] = msz[par] - f_ov if mult == 1 else 0
      tg[par] = 0 if mult == 1 else msz[par] - f_ov
      pos = (mult == 1 and off_o > 0) or (mult == -1 and off_o < 0)
      neg = (mult == 1 and off_o < 0) or (mult == -1 and off_o > 0)
      start[ortho] = msz[ortho] - f_o if pos else 0
      tg[ortho] = msz[ortho] - f_o if neg else 0
      fine = [fine_x, fine_y]
      if nd == 3:
        off_z, f_z, fine_z = int(nb[8]), int(nb[9]), int(nb[10])
        zpos = (mult == 1 and off_z > 0) or (mult == -1 and off_z < 0)
        zneg = (mult == 1 and off_z < 0) or (mult == -1 and off_z > 0)
        start[0] = msz[0] - f_z if zpos else 0
        tg[0] = msz[0] - f_z if zneg else 0
        fine.append(fine_z)
      assert min(start) >= 0 and min(tg) >= 0, 'out of contract'
      m1 = f32(mult) * np.asarray(flow[:, flow_idx], f32)
      if nd == 2:
        upd, nr, b = compose64(m1[:, None], [0] + start, st, x[:, nbor][:, None], (0, 0, 0), st,
                               'constant')
        upd, nr = upd[:, 0], nr[0]
      else:
        upd, nr, b = compose64(m1, start, st, x[:, nbor], (0, 0, 0), st, 'constant')
      upd = upd + mult * np.array(fine, np.float64).reshape((nd,) + (1,) * nd)
      fin = upd[np.isfinite(upd)]
      big = max(big, b, float(np.abs(fin).max()) if fin.size else 0.0)
      sl = tuple(slice(o, o + s) for o, s in zip(tg, upd.shape[1:]))
      prev = canvas[(slice(None),) + sl]
      if stats is not None:
        stats['signs'].add((int(np.sign(off_o)), mult, dim))
        if nd == 3:
          stats['signs_z'].add((int(np.sign(off_z)), mult))
        stats['cropped'] += any(o + s > m for o, s, m in zip(tg, upd.shape[1:], msz))
        inside = np.zeros(ext, bool)
        inside[crop] = True
        keep = np.isnan(upd) & ~np.isnan(prev)
        one = keep.any(axis=0) & ~keep.all(axis=0) & (~np.isnan(upd)).any(axis=0)
        stats['survive_one'] += int((one & inside[sl]).sum())
        for ax in range(nd):
          idx = np.arange(upd.shape[1 + ax]) + start[ax]
          shape = [1] * nd
          shape[ax] = -1
          q = idx.reshape(shape) + m1[nd - 1 - ax].astype(np.float64) / st[ax]
          with np.errstate(invalid='ignore'):
            if (q < 0).any():
              stats['out'].add((ax, 'lo'))
            if (q > msz[ax] - 1).any():
              stats['out'].add((ax, 'hi'))
            stats['last'] += int((q == msz[ax] - 1).sum())
      canvas[(slice(None),) + sl] = np.where(np.isnan(upd), prev, upd)
      cnear[sl] |= nr
    out[:, t] = canvas[(slice(None),) + crop]
    near[t] = cnear[crop]
    if stats is not None:
      stats['all_nan_tiles'] += bool(np.isnan(out[:, t]).all())
  return out, near, big


def target_atol(nd, big):
  """compose_atol (the sampled coordinate is a sum of T float32 products, T = 4
  bilinear / 8 trilinear, then the difference of two coordinates) plus one more
  rounding for the fine offset added to it: (T + 4) 2^-24 M."""
  return compose_atol(nd, big) + 2.0**-24 * big


_REFS = {}


def target_refs(name):
  """(float32 oracle, float64 reference, near, M) of one case; computed once."""
  if name not in _REFS:
    c = target_cases()[name]
    with np.errstate(all='ignore'):
      want32 = maps_oracle.target_mesh_all(c['nbors'], c['x'], c['fx'], c['fy'], c['stride'])
      want64, near, big = target64(c['nbors'], c['x'], c['fx'], c['fy'], c['stride'])
    _frozen(want32, want64, near)
    _REFS[name] = (want32, want64, near, big)
  return _REFS[name]


def _same_nonfinite(got, want, where, msg):
  np.testing.assert_array_equal(np.isnan(got)[where], np.isnan(want)[where], err_msg=msg)
  for inf in (np.inf, -np.inf):
    np.testing.assert_array_equal((got == inf)[where], (want == inf)[where], err_msg=msg)


def check_target(got, name, tiles=None):
  """`got` ([ncomp, tiles, *mesh]) against (a) the float32 oracle: same NaN /
  inf pattern, values within (T + 4) 2^-24 M; (b) target64: the same outside
  `near`, with `near` capped at max(2, 1e-3 n) nodes.  Returns (largest
  |got - float32 oracle|, largest |got - float64|, bound)."""
  want32, want64, near, big = target_refs(name)
  if tiles is not None:
    want32, want64, near = want32[:, tiles], want64[:, tiles], near[tiles]
  got = np.asarray(got)
  nd = want32.shape[0]
  atol = target_atol(nd, big)
  assert got.shape == want32.shape and got.dtype == np.float32, name
  everywhere = np.ones(got.shape, bool)
  _same_nonfinite(got, want32, everywhere, name)
  fin = np.isfinite(want32)
  d32 = float(np.abs(got[fin].astype(np.float64) - want32[fin]).max()) if fin.any() else 0.0
  assert d32 <= atol, f'{name}: |got - float32 oracle| = {d32:.4g} > {atol:.4g}'
  assert near.sum() <= max(2, 1e-3 * near.size), f'{name}: {int(near.sum())} queries next to a node'
  keep = np.broadcast_to(~near, got.shape)
  _same_nonfinite(got, want64, keep, name)
  fin = np.isfinite(got) & np.isfinite(want64)
  d64 = float(np.abs(got[fin] - want64[fin]).max()) if fin.any() else 0.0
  assert d64 <= atol, f'{name}: |got - float64| = {d64:.4g} > {atol:.4g} (M = {big:.6g})'
  return d32, d64, atol


def _target_fn(case):
  from sofima_amd import stitch_elastic
  return stitch_elastic.TargetMeshFn(case['nbors'], case['fx'], case['fy'], case['stride'])


# ---------------------------------------------------------------------------
# Target mesh: GPU tests
# ---------------------------------------------------------------------------
TARGET_CASE_NAMES = (
    'g13_40x5', 'g13_5x40', 'g22_15x31', 'g22_15x47', 'g22_16x16', 'g22_16x48', 'g22_17x33',
    'g22_17x33_nan', 'g22_17x49_nan', 'g31_40x5', 'g31_5x40', 'isolated_tile', 'large_amp',
    'nonfinite_x', 'vol12_thin', 'vol12_z0', 'vol12_zneg', 'vol12_zpos', 'vol21_thin',
    'vol21_z0', 'vol21_zneg', 'vol21_zpos', 'zero_flow')     # == sorted(target_cases())


@pytest.mark.parametrize('name', TARGET_CASE_NAMES)
def test_target_mesh_edges(gpu, name):
  """TargetMeshFn(...)(x) on every case: equal NaN / inf patterns and the
  derived bound against both references, and bit for bit against the float32
  oracle: the kernel follows the oracle's operation order term by term and is
  built without FMA contraction, so every IEEE operation rounds alike."""
  case = target_cases()[name]
  got = np.array(_target_fn(case)(case['x']))
  d32, d64, atol = check_target(got, name)
  print(f'{name}: |got - f32 oracle| = {d32:.3g}, |got - f64| = {d64:.3g}, allowed {atol:.3g}')
  np.testing.assert_array_equal(got, target_refs(name)[0])


def test_target_mesh_edge_values(gpu):
  """What the special cases are there for, stated on the kernel's output."""
  cases = target_cases()
  run = lambda name: np.array(_target_fn(cases[name])(cases[name]['x']))
  # four -1 rows: nothing pasted
  got = run('isolated_tile')
  assert np.isnan(got[:, 2]).all() and np.isfinite(got[:, 0]).any()
  # zero flow, mult = +1 strip of tile 1 (left neighbour 0): the query of its
  # last column sits ON the neighbour's last node -> NaN; the columns before
  # are the neighbour's own displacements plus the fine offset
  got = run('zero_flow')
  case = cases['zero_flow']
  nb = case['nbors'][1, 0]
  assert nb[0] == 0 and nb[1] == 0 and nb[2] == 0
  my, mx = case['x'].shape[-2:]
  ov = int(nb[4])
  f_o = min(int(nb[3]), my - ov)     # the rows below belong to the y strip pasted later
  assert np.isnan(got[:, 1, :f_o, ov - 1]).all()
  want = case['x'][0, 0, :f_o, mx - ov:mx - 1] + f32(nb[5])
  np.testing.assert_allclose(got[0, 1, :f_o, :ov - 1], want, rtol=0,
                             atol=target_atol(2, target_refs('zero_flow')[3]))
  # one NaN flow component makes the query NaN: both components of the update
  # are NaN and the earlier update survives in both
  got = run('g22_17x33_nan')
  case = cases['g22_17x33_nan']
  my, mx = case['x'].shape[-2:]
  ov = 6
  f_ortho_y = int(case['nbors'][0, 3, 3])
  assert f_ortho_y == mx          # offset 0: the strip covers the whole axis
  y0, x0 = my - ov, mx - ov
  only_x = _target_fn(dict(case, nbors=np.where(
      np.arange(4)[None, :, None] == 1, case['nbors'], -1)))(case['x'])
  only_x = np.array(only_x)
  for dy, dx in ((1, 1), (2, 2), (0, 4)):     # NaN in one component of the later flow
    np.testing.assert_array_equal(got[:, 0, y0 + dy, x0 + dx], only_x[:, 0, y0 + dy, x0 + dx])
    assert np.isfinite(only_x[:, 0, y0 + dy, x0 + dx]).all()
  assert np.isnan(got[:, 0, y0 + 3, x0 + 3]).all()      # NaN in both updates
  # out of range on every side
  got = run('large_amp')
  assert 0.05 < np.isnan(got[:, :, :, :6]).mean() < 0.95


@pytest.mark.parametrize('name', SINGLE_TILE_CASES)
def test_compute_target_mesh_single_tile(gpu, name):
  """compute_target_mesh (n_eval = 1): one row block against all meshes, for
  every tile."""
  from sofima_amd import stitch_elastic
  case = target_cases()[name]
  want32 = target_refs(name)[0]
  for t in range(case['nbors'].shape[0]):
    one = stitch_elastic.compute_target_mesh(case['nbors'][t], case['x'], case['fx'],
                                             case['fy'], case['stride'])
    assert one.shape == want32[:, t].shape
    check_target(one[:, None], name, tiles=[t])
    np.testing.assert_array_equal(one, want32[:, t])


def prev_fn_config(variant, stride_yx):
  from sofima_amd import mesh
  kw = dict(dt=0.001, gamma=0.0, k0=0.02, k=0.1, stride=tuple(stride_yx[::-1]), num_iters=20,
            max_iters=40, stop_v_max=1e-9, dt_max=100, prefer_orig_order=True,
            start_cap=0.1, final_cap=10.0, remove_drift=(variant == 'fire_drift'))
  if variant == 'verlet':
    kw.update(fire=False, gamma=0.5, dt=0.05, start_cap=10.0)
  return mesh.IntegrationConfig(**kw)


@pytest.mark.parametrize('variant', ['fire_drift', 'fire', 'verlet'])
@pytest.mark.parametrize('name', PREV_FN_CASES)
def test_target_mesh_as_prev_fn(gpu, name, variant):
  """Tiled in-plane relaxation (x >= 40 and y >= 4 nodes) with the native
  prev_fn on padded flows, NaN corners and block-edge geometries: the
  strips-only target mesh over the 16 x 16 block list, fused with the
  integrator, == SFM_MESH_FUSE_TARGET=0 bit for bit; it follows the untiled
  path and the oracle driven by the float32 target-mesh oracle."""
  from sofima_amd import _abi, mesh
  case = target_cases()[name]
  assert case['x'].shape[-1] >= 40 and case['x'].shape[-2] >= 4
  stride = case['stride']
  cfg = prev_fn_config(variant, stride)
  fn = _target_fn(case)
  x0 = case['x']
  a = mesh.relax_mesh(x0, None, cfg, prev_fn=fn)
  with _abi.option('SFM_MESH_FUSE_TARGET', 0):
    b = mesh.relax_mesh(x0, None, cfg, prev_fn=fn)
  np.testing.assert_array_equal(np.array(a[0]), np.array(b[0]))
  assert a[1] == b[1] and a[2] == b[2]
  with _abi.option('SFM_MESH_TILED', 0):
    c = mesh.relax_mesh(x0, None, cfg, prev_fn=fn)
  want = mesh_oracle.relax_mesh(
      x0, None, cfg, prev_fn=lambda xx: maps_oracle.target_mesh_all(
          case['nbors'], xx, case['fx'], case['fy'], stride))
  for other in (c, want):
    ox = np.array(other[0])
    assert a[2] == other[2]
    np.testing.assert_allclose(np.array(a[0]), ox, atol=1e-3 * np.abs(ox).max())
    np.testing.assert_allclose(a[1], other[1], rtol=1e-3)


# ---------------------------------------------------------------------------
# Tile mesh force
# ---------------------------------------------------------------------------
TILE_GRIDS = ((1, 1), (1, 5), (5, 1), (2, 3), (17, 19))
TILE_VARIANTS = ('plain', 'missing', 'inf', 'x_nonfinite', 'saturated')


def tile_force_case(ncomp, nz, ny, nx, variant):
  """(x, cx, cy), each [ncomp, nz, ny, nx] float32."""
  rng = np.random.default_rng((((ncomp * 7 + nz) * 31 + ny) * 37 + nx) * 5 + TILE_VARIANTS.index(variant))
  shape = (ncomp, nz, ny, nx)
  x = (rng.standard_normal(shape) * 40).astype(f32)
  cx = (rng.standard_normal(shape) * 6).astype(f32)
  cy = (rng.standard_normal(shape) * 6).astype(f32)
  cx[0] += 100
  cy[1] += 100
  pick = lambda p: rng.random(shape[1:]) < p
  if variant == 'missing':        # a missing tile: NaN in every component
    cx[:, pick(0.25)] = np.nan
    cy[:, pick(0.25)] = np.nan
    cx[:, :, :, nx // 2] = np.nan
    cy[:, 0, 0, 0] = np.nan
  elif variant == 'inf':          # no estimate met the criteria
    cx[:, pick(0.2)] = np.inf
    cy[:, pick(0.2)] = np.inf
    cx[0, pick(0.1)] = -np.inf
    cy[ncomp - 1, pick(0.1)] = -np.inf
  elif variant == 'x_nonfinite':
    x[:, pick(0.1)] = np.nan
    x[0, pick(0.1)] = np.inf
    x[1, pick(0.1)] = -np.inf
    x[ncomp - 1, 0, 0, 0] = np.nan
  elif variant == 'saturated':
    # runs of -inf: neighbouring pair terms are both +FLT_MAX and cancel in the
    # node between them; +inf next to -inf: they add up and overflow
    cx[:, :, :, : max(1, nx - 2)] = -np.inf
    cy[:, :, : max(1, ny - 2), :] = -np.inf
    if nx >= 4:
      cx[:, :, :, 1] = np.inf
    if ny >= 4:
      cy[1, :, 2, :] = np.inf
  return x, cx, cy


def tile_force64(x, cx, cy):
  """The tile-mesh force (stitch_rigid.py:330-473) from the definition, in
  double: every pair (i, i + 1) along x / y contributes
  t = nan_to_num((x[i + 1] - x[i]) - c[i]) (NaN -> 0, beyond +-FLT_MAX ->
  +-FLT_MAX) to node i and -t to node i + 1, per component and section.

  Returns (force, bound, saturated).  Bound: a float32 pair term carries two
  roundings, of d = x[i + 1] - x[i] and of d - c: at most 2^-24 (|d| + |t|);
  the four terms of a node are added to 0 one after the other, the first
  exactly, each of the three further sums rounding by at most 2^-24 of a
  partial sum <= sum |t|.  Per node: 2^-24 (sum |d| + 4 sum |t|), times
  (1 + 2^-20) for the second-order terms.  `saturated` marks nodes with a
  term at +-FLT_MAX, where float32 partial sums may overflow: those are
  compared with the float32 oracle alone."""
  x = np.asarray(x, f32).astype(np.float64)
  force = np.zeros(x.shape)
  abs_t = np.zeros(x.shape)
  abs_d = np.zeros(x.shape)
  sat = np.zeros(x.shape, bool)
  for c_arr, axis in ((cx, -1), (cy, -2)):
    c_arr = np.asarray(c_arr, f32).astype(np.float64)
    hi = [slice(None)] * 4
    lo = [slice(None)] * 4
    hi[axis], lo[axis] = slice(1, None), slice(None, -1)
    hi, lo = tuple(hi), tuple(lo)
    with np.errstate(invalid='ignore', over='ignore'):
      d = x[hi] - x[lo]
      t = d - c_arr[lo]
    d = np.clip(np.nan_to_num(d, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX), -FLT_MAX, FLT_MAX)
    t = np.clip(np.nan_to_num(t, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX), -FLT_MAX, FLT_MAX)
    s = np.abs(t) >= FLT_MAX
    force[lo] += t
    force[hi] -= t
    for side in (lo, hi):
      abs_t[side] += np.abs(t)
      abs_d[side] += np.abs(d)
      sat[side] |= s
  bound = 2.0**-24 * (abs_d + 4 * abs_t) * (1 + 2.0**-20)
  return force, bound, sat


def check_tile_force(got, x, cx, cy, msg):
  """Bit for bit with the float32 oracle (same operation order); within the
  derived bound of tile_force64 wherever no term saturates.  Returns the
  largest error in units of the bound."""
  ncomp = x.shape[0]
  oracle = stitch_oracle.elastic_tile_mesh if ncomp == 2 else stitch_oracle.elastic_tile_mesh_3d
  with np.errstate(all='ignore'):
    want32 = oracle(x, cx, cy)
  got = np.asarray(got)
  assert got.shape == x.shape and got.dtype == np.float32, msg
  np.testing.assert_array_equal(got, want32, err_msg=msg)
  want64, bound, sat = tile_force64(x, cx, cy)
  assert not np.isnan(got).any(), msg            # nan_to_num: a force is never NaN
  ok = ~sat
  assert np.isfinite(got[ok]).all(), msg
  err = np.abs(got[ok].astype(np.float64) - want64[ok])
  assert (err <= bound[ok]).all(), f'{msg}: {err.max():.4g} beyond the bound'
  with np.errstate(invalid='ignore', divide='ignore'):
    used = np.where(bound[ok] > 0, err / bound[ok], 0.0)
  return float(used.max()) if used.size else 0.0


def tile_force_params():
  return [(c, z, y, x) for c in (2, 3) for z in (1, 3) for (y, x) in TILE_GRIDS]


@pytest.mark.parametrize('ncomp,nz,ny,nx', tile_force_params())
def test_tile_mesh_force_edges(gpu, ncomp, nz, ny, nx):
  from sofima_amd import stitch_rigid
  fn = stitch_rigid.elastic_tile_mesh if ncomp == 2 else stitch_rigid.elastic_tile_mesh_3d
  for variant in TILE_VARIANTS:
    x, cx, cy = tile_force_case(ncomp, nz, ny, nx, variant)
    got = np.array(fn(x, cx, cy))
    check_tile_force(got, x, cx, cy, f'[{ncomp}, {nz}, {ny}, {nx}] {variant}')
  if (ny, nx) == (1, 1):
    assert not got.any()            # a single tile has no pair


def coarse_mesh_cases():
  """{name: (cx, cy)} [2, 1, y, x]: offsets to the right / lower neighbour, NaN
  where there is none (last column of cx, last row of cy)."""
  out = {}
  for name, (ny, nx) in (('1x1', (1, 1)), ('1x3', (1, 3)), ('3x1', (3, 1)), ('2x3_nan', (2, 3))):
    rng = np.random.default_rng(ny * 10 + nx)
    cx = (rng.standard_normal((2, 1, ny, nx)) * 4).astype(f32)
    cy = (rng.standard_normal((2, 1, ny, nx)) * 4).astype(f32)
    cx[0] += 90
    cy[1] += 110
    cx[:, :, :, -1] = np.nan
    cy[:, :, -1, :] = np.nan
    if name == '2x3_nan':
      cx[:, :, :, 1] = np.nan       # no estimate between columns 1 and 2
      cy[:, :, :, 1] = np.nan       # the middle column hangs on its left neighbours only
    out[name] = _frozen(cx, cy)
  return out


def coarse_mesh_config():
  from sofima_amd import mesh
  return mesh.IntegrationConfig(dt=0.001, gamma=0.0, k0=0.0, k=0.1, stride=(1, 1),
                                num_iters=1000, max_iters=20000, stop_v_max=0.001, dt_max=100)


@pytest.mark.parametrize('name', ['1x1', '1x3', '3x1', '2x3_nan'])
def test_optimize_coarse_mesh_small_grids(gpu, name):
  from sofima_amd import mesh, stitch_rigid
  cx, cy = coarse_mesh_cases()[name]
  cfg = coarse_mesh_config()
  want = stitch_oracle.optimize_coarse_mesh(cx, cy, cfg)
  got = stitch_rigid.optimize_coarse_mesh(cx, cy, cfg)
  assert got.shape == want.shape and got.dtype == np.float32
  np.testing.assert_allclose(got, want, atol=1e-3)
  gx, ge, gt = mesh.relax_mesh(np.zeros_like(cx), None, cfg,
                               mesh_force=mesh.TileMeshForce(cx, cy))
  wx, we, wt = mesh_oracle.relax_mesh(
      np.zeros_like(cx), None, cfg,
      mesh_force=lambda x, *a, **k: stitch_oracle.elastic_tile_mesh(x, cx, cy))
  assert gt == wt and len(ge) == len(we)
  np.testing.assert_allclose(np.array(gx), wx, atol=1e-3)
  if name == '1x1':
    assert not got.any()


# ---------------------------------------------------------------------------
# Range mask
# ---------------------------------------------------------------------------
RANGE_SHAPES = ((1, 1), (1, 9), (9, 1), (3, 5), (33, 257))
RANGE_SIZES = (1, 2, 3, 10, 13, 31)     # 31: several reflection periods of the small images
LIMIT_FORMS = {'int': int, 'float': float, 'float32': np.float32, 'float64': np.float64,
               'int64': np.int64}


def range_image(shape, dtype, seed=0):
  """Random image with flat patches, so that small windows have range 0."""
  rng = np.random.default_rng(seed + shape[0] * 1000 + shape[1])
  if dtype == np.uint8:
    img = rng.integers(0, 256, shape).astype(np.uint8)
  elif dtype == np.uint16:
    img = rng.integers(0, 65536, shape).astype(np.uint16)
  else:
    img = (rng.standard_normal(shape) * 20).astype(f32)
  if shape[0] > 8 and shape[1] > 100:
    img[5:20, 40:90] = img[5, 40]
    img[25:, :30] //= 16 if dtype != np.float32 else 1
  return img


def spike_image(values, dtype, spacing=8):
  """Zeros with isolated pixels `values`, `spacing` apart: a window of size
  <= spacing holds at most one, so its range is that value exactly."""
  img = np.zeros((spacing * 2 + 1, spacing * (len(values) + 1) + 1), dtype)
  for i, v in enumerate(values):
    img[spacing, spacing * (i + 1)] = v
  return img


def _around_all(values):
  """The float32 nearest to each value and its two neighbours on either side."""
  return [v for c in values for v in around(c)]


def f32_limit_cases():
  """[(image, limit)] float32 spike images whose window ranges sit on
  float32(L) and one ulp to either side, for limits L that float32 rounds down
  (0.7), rounds up (0.1) and holds exactly (2.5), each as a Python float, a
  float32 and a float64 scalar."""
  out = []
  for L in (0.7, 0.1, 2.5, 40.3):
    c = f32(L)
    vals = [np.nextafter(c, f32(-np.inf)), c, np.nextafter(c, f32(np.inf))]
    img = spike_image(vals, f32)
    for form in ('float', 'float32', 'float64'):
      out.append((img, LIMIT_FORMS[form](L)))
  return out


def u16_limit_case():
  """uint16 windows of range 3 (and 2, 4) against the Python float 3.0000001,
  which float32 rounds to 3: NumPy compares an integer image with a Python
  float in double."""
  return spike_image([2, 3, 4], np.uint16) + np.uint16(1000), 3.0000001


def _run_mask(img, limit, size, extra=None):
  from sofima_amd import stitch_rigid
  out = stitch_rigid.range_mask(img, limit, size, extra)
  assert out.dtype.is_floating_point is False and tuple(out.shape) == tuple(np.shape(img))
  return out.cpu().numpy().astype(bool)


def check_range_mask(img, limit, size):
  want = stitch_oracle.range_mask(img, limit, size)
  got = _run_mask(img, limit, size)
  np.testing.assert_array_equal(
      got, want, err_msg=f'{img.dtype} {img.shape} size {size} limit {limit!r} ({type(limit).__name__})')
  return want


@pytest.mark.parametrize('dtype', [np.uint8, np.uint16, np.float32])
def test_range_mask_shapes_and_filter_sizes(gpu, dtype):
  masked = kept = 0
  for shape in RANGE_SHAPES:
    img = range_image(shape, dtype)
    for size in RANGE_SIZES:
      for limit in (30, 200.5) if dtype != np.uint16 else (3000, 60000.5):
        want = check_range_mask(img, limit, size)
        masked += int(want.sum())
        kept += int((~want).sum())
  assert masked > 1000 and kept > 1000


def test_range_mask_uint8_limits(gpu):
  """Constant images, ranges exactly on the limit, limits outside 0 .. 255,
  every limit in every scalar form."""
  flat = np.full((9, 12), 77, np.uint8)
  assert not check_range_mask(flat, 0, 3).any()           # 0 < 0
  assert check_range_mask(flat, 1e-30, 3).all()           # 0 < 1e-30
  steps = spike_image([24, 25, 26, 254, 255], np.uint8)
  for size in (1, 2, 3, 8):
    for value in (-1, 0, 0.5, 25, 25.5, 26, 255, 256, 1000):
      for form, cast in LIMIT_FORMS.items():
        if form in ('int', 'int64') and value != int(value):
          continue
        check_range_mask(steps, cast(value), size)
        check_range_mask(range_image((33, 257), np.uint8, 5), cast(value), size)
  want = check_range_mask(steps, 25, 3)
  assert want[8, 8] and not want[8, 16] and not want[8, 24]   # 24 < 25, 25 !< 25


def test_range_mask_float32_limit_forms(gpu):
  """Window ranges on float32(L) and one ulp beside it.  NumPy rounds a Python
  float or a float32 scalar to float32 before it compares with a float32
  image, a float64 scalar compares in double: for L = 0.7 (float32(L) < L) the
  range float32(L) is masked by np.float64(0.7) and not by 0.7."""
  differ = 0
  for img, limit in f32_limit_cases():
    for size in (1, 3, 8):
      want = check_range_mask(img, limit, size)
      assert want.any() and (size == 1 or not want.all())   # size 1: every range is 0
    differ += int((stitch_oracle.range_mask(img, f32(limit), 3) !=
                   stitch_oracle.range_mask(img, limit, 3)).any())
  assert differ >= 2
  # a random image against limits taken from its own window ranges
  from scipy import ndimage
  img = range_image((33, 257), np.float32, 9)
  rng_ = ndimage.maximum_filter(img, 3) - ndimage.minimum_filter(img, 3)
  for v in np.unique(rng_)[[5, 100, 1000, -3]]:
    for limit in (float(v), v, np.float64(v), float(np.nextafter(v, f32(np.inf))),
                  float(v) * (1 + 2.0**-30)):
      check_range_mask(img, limit, 3)


def test_range_mask_uint16_python_float_limit(gpu):
  img, limit = u16_limit_case()
  for size in (1, 3, 8):
    want = check_range_mask(img, limit, size)
    assert want[8, 16]                     # the range-3 window: 3 < 3.0000001
  for form in ('float32', 'float64'):      # float32(3.0000001) == 3: not masked
    check_range_mask(img, LIMIT_FORMS[form](limit), 3)
  check_range_mask(img, 3, 3)
  check_range_mask(img, np.int64(4), 3)
  big = spike_image([65535, 65534, 1], np.uint16)
  for limit in (65535, 65535.5, 65536, np.float32(65535), np.float64(65534.99)):
    check_range_mask(big, limit, 2)


def test_range_mask_infinite_pixels(gpu):
  """max - min is inf next to an inf pixel and NaN (never below a limit)
  where a window holds both signs or nothing but one infinity."""
  img = range_image((33, 257), np.float32, 3)
  img[3, 3] = np.inf
  img[10, 100] = -np.inf
  img[20, 200:203] = np.inf
  img[21, 201] = -np.inf
  img[28:33, 250:257] = np.inf         # whole windows of +inf: inf - inf
  for size in (1, 2, 3, 10):
    for limit in (30, np.inf, np.float64(1e300)):
      with np.errstate(invalid='ignore'):
        check_range_mask(img, limit, size)


def test_range_mask_extra_mask_forms(gpu):
  import torch
  from sofima_amd import _dev
  img = range_image((33, 257), np.uint8, 4)
  rng = np.random.default_rng(4)
  extra = rng.random(img.shape) < 0.2
  want = stitch_oracle.range_mask(img, 60, 3) | extra
  assert (want != extra).any() and not want.all()
  odd = extra.astype(np.uint8) * rng.choice(np.array([1, 2, 128, 255], np.uint8), img.shape)
  forms = [extra, odd, torch.from_numpy(extra), torch.from_numpy(odd).to(gpu),
           _dev.DeviceArray(torch.from_numpy(odd).to(gpu)),
           _dev.DeviceArray(torch.from_numpy(extra.astype(np.float32)).to(gpu))]
  for e in forms:
    np.testing.assert_array_equal(_run_mask(img, 60, 3, e), want)
  # the image itself as a device tensor / DeviceArray
  t = torch.from_numpy(img).to(gpu)
  np.testing.assert_array_equal(_run_mask(t, 60, 3, extra), want)
  f = range_image((33, 257), np.float32, 4)
  wf = stitch_oracle.range_mask(f, np.float64(17.3), 3)
  got = _run_mask(_dev.DeviceArray(torch.from_numpy(f).to(gpu)), np.float64(17.3), 3)
  np.testing.assert_array_equal(got, wf)
  # a torch dtype NumPy has no name for is narrowed to float32 like any other
  b = torch.from_numpy(f).to(gpu).to(torch.bfloat16)
  np.testing.assert_array_equal(_run_mask(b, 17.5, 3),
                                stitch_oracle.range_mask(b.float().cpu().numpy(), 17.5, 3))


def test_range_mask_errors(gpu):
  from sofima_amd import _abi, stitch_rigid
  img = range_image((9, 12), np.uint8)
  with pytest.raises(ValueError, match='shapes differ'):
    stitch_rigid.range_mask(img, 10, 3, np.zeros((9, 11), bool))
  with pytest.raises(ValueError, match='2-d'):
    stitch_rigid.range_mask(np.zeros((2, 9, 12), np.uint8), 10, 3)
  with pytest.raises(_abi.SofimaAmdError, match='filter size'):
    stitch_rigid.range_mask(img, 10, 0)
