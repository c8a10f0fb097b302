"""The unit list of the build: a .hip that SOURCES does not name is not built."""
import os
import re

from sofima_amd import _build


def test_every_unit_is_listed_and_exists():
  on_disk = sorted(f for f in os.listdir(_build.CSRC) if f.endswith('.hip'))
  assert on_disk == sorted(_build.SOURCES)


def test_matrix_core_units_take_the_matrix_core_flags():
  """MFMA_UNITS (the timing and ablation builds go by it) = the files of the path, one
  geometry unit per entry of SFM_MFMA_GEOMETRIES, each naming its own geometry."""
  on_disk = sorted(f for f in os.listdir(_build.CSRC)
                   if f.endswith('.hip') and f.startswith(('sfm_mfma', 'sfm_xcorr_mfma')))
  assert on_disk == sorted(_build.MFMA_UNITS)
  assert all(_build.SOURCES[u] is _build.SOURCES['sfm_mfma_host.hip'] for u in on_disk)
  text = open(os.path.join(_build.CSRC, 'sfm_mfma.h')).read()
  body = re.search(r'#define SFM_MFMA_GEOMETRIES\(X\)((?:.*\\\n)*.*)\n', text).group(1)
  listed = re.findall(r'X\((\d+), (\d+)\)', body)
  assert len(listed) == 9
  for nca, nce in listed:
    unit = 'sfm_mfma_g%sx%s.hip' % (nca, nce)
    assert unit in _build.MFMA_UNITS
    assert 'SFM_MFMA_GEOMETRY_UNIT(%s, %s)' % (nca, nce) in open(
        os.path.join(_build.CSRC, unit)).read()
  assert len(on_disk) == len(listed) + 2


def test_warp_units_are_built_without_contraction():
  """NDWARP_UNITS = the kernel units of the map_coordinates family on disk; each names
  its own (order, dimension) and only that; together they instantiate every entry of
  SFM_NDWARP_UNITS once, whole or as its three maps and the rest; all of them, and
  the host unit, carry -ffp-contract=off."""
  on_disk = sorted(f for f in os.listdir(_build.CSRC)
                   if f.endswith('.hip') and f.startswith('sfm_ndwarp'))
  assert on_disk == sorted(_build.NDWARP_UNITS)
  for unit in on_disk + ['sfm_warp.hip']:
    assert '-ffp-contract=off' in _build.SOURCES[unit], unit
  text = open(os.path.join(_build.CSRC, 'sfm_ndwarp.h')).read()
  body = re.search(r'#define SFM_NDWARP_UNITS\(X\)((?:.*\\\n)*.*)\n', text).group(1)
  listed = re.findall(r'X\((\d), (\d)\)', body)
  assert sorted(listed) == sorted((str(o), str(d)) for o in (0, 2, 3, 4, 5) for d in (2, 3))
  whole = ['AbsoluteMap', 'IMAGE', 'RelativeMapArgs<double>', 'RelativeMapArgs<float>']
  parts = {}
  for unit in on_disk:
    name = re.fullmatch(r'sfm_ndwarp_o(\d)(?:d(\d))?(?:_[a-z0-9]+)?\.hip', unit)
    assert name, unit
    code = [l for l in open(os.path.join(_build.CSRC, unit)).read().split('\n')
            if l and not l.startswith(('//', '#include'))]
    assert code, unit
    for line in code:
      m = re.fullmatch(r'SFM_NDWARP_(UNIT|IMAGE_UNIT|MAP_UNIT)\((\d), (\d)(?:, ([\w<>]+))?\)', line)
      assert m, (unit, line)
      kind, order, dim, map_type = m.groups()
      assert order == name.group(1) and name.group(2) in (None, dim), (unit, line)
      assert (map_type is not None) == (kind == 'MAP_UNIT'), (unit, line)
      parts.setdefault((order, dim), []).extend(
          whole if kind == 'UNIT' else [map_type or 'IMAGE'])
  assert sorted(parts) == sorted(listed)
  for entry, got in parts.items():
    assert sorted(got) == whole, entry


def test_job_count_is_bounded(monkeypatch):
  for cpus in (None, 1, 8, 16, 17, 384):
    monkeypatch.setattr(os, 'cpu_count', lambda cpus=cpus: cpus)
    for env in (None, '', '0', '-3', '1', '7', '16', '17', '4096', 'many'):
      if env is None:
        monkeypatch.delenv('MAX_JOBS', raising=False)
      else:
        monkeypatch.setenv('MAX_JOBS', env)
      n = _build.jobs()
      assert 1 <= n <= 16, (cpus, env, n)
      if env in ('1', '7', '16'):
        assert n == int(env)
      elif env in (None, '', 'many'):
        assert n == max(1, min(cpus or 1, 16))
