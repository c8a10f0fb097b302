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
