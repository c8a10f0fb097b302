"""Builds libsofima_amd.so (HIP, gfx950) and the C oracle helpers in-tree."""
from __future__ import annotations

import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, 'csrc')
LIB_DIR = os.path.join(PKG_DIR, 'lib')
LIB_PATH = os.path.join(LIB_DIR, 'libsofima_amd.so')
OBJ_DIR = os.path.join(PKG_DIR, 'build')

# SFM_MFMA_TIMING / SFM_MFMA_FLAGS: instrumentation and tuning experiments, for the
# units of the matrix-core correlation path
_MFMA = ((['-DSFM_MFMA_TIMING'] if os.environ.get('SFM_MFMA_TIMING') else []) +
         os.environ.get('SFM_MFMA_FLAGS', '').split())

# The units of the matrix-core correlation path (csrc/sfm_mfma.h lists them; one unit
# per chunk geometry of the correlation kernel): they all take the _MFMA flags
MFMA_UNITS = ('sfm_mfma_g10x11.hip', 'sfm_mfma_g20x11.hip', 'sfm_mfma_g15x11.hip',
              'sfm_mfma_g8x9.hip', 'sfm_mfma_g7x8.hip', 'sfm_mfma_g6x7.hip',
              'sfm_mfma_g5x6.hip', 'sfm_mfma_g4x5.hip', 'sfm_mfma_g3x4.hip',
              'sfm_xcorr_mfma.hip', 'sfm_mfma_host.hip')

# The units that hold the kernels of the map_coordinates family (csrc/sfm_ndwarp.h
# lists them: one unit per spline order and dimension, the 3-D ones of orders 4 and 5
# cut once more by map accessor).  Double arithmetic in SciPy's operation order: FMA
# contraction is disabled in all of them, as in their host unit sfm_warp.hip.
_NDWARP = ['-ffp-contract=off']
NDWARP_UNITS = ('sfm_ndwarp_o0.hip', 'sfm_ndwarp_o2d2.hip', 'sfm_ndwarp_o2d3.hip',
                'sfm_ndwarp_o3d2.hip', 'sfm_ndwarp_o3d3.hip', 'sfm_ndwarp_o4d2.hip',
                'sfm_ndwarp_o4d3_abs.hip', 'sfm_ndwarp_o4d3_rel32.hip',
                'sfm_ndwarp_o4d3_rel64.hip', 'sfm_ndwarp_o4d3_image.hip',
                'sfm_ndwarp_o5d2.hip', 'sfm_ndwarp_o5d3_abs.hip', 'sfm_ndwarp_o5d3_rel32.hip',
                'sfm_ndwarp_o5d3_rel64.hip', 'sfm_ndwarp_o5d3_image.hip')

# Translation units and their extra flags, the slowest to compile first, as measured
# one unit at a time (profiles/build_time.txt).  The mesh kernels follow the
# reference's f32 operation order, so FMA contraction is disabled there.
SOURCES = {
    'sfm_ndwarp_o3d3.hip': _NDWARP,          # 61 s
    'sfm_ndwarp_o2d3.hip': _NDWARP,
    'sfm_ndwarp_o0.hip': _NDWARP,
    'sfm_ndwarp_o4d3_abs.hip': _NDWARP,      # 24 s
    'sfm_ndwarp_o5d3_rel32.hip': _NDWARP,
    'sfm_ndwarp_o4d3_rel64.hip': _NDWARP,
    'sfm_ndwarp_o5d3_rel64.hip': _NDWARP,
    'sfm_ndwarp_o5d3_abs.hip': _NDWARP,
    'sfm_ndwarp_o4d3_rel32.hip': _NDWARP,
    'sfm_ndwarp_o5d2.hip': _NDWARP,
    'sfm_mfma_g10x11.hip': _MFMA,            # 17 s
    'sfm_ndwarp_o4d2.hip': _NDWARP,
    'sfm_ndwarp_o3d2.hip': _NDWARP,
    'sfm_xcorr.hip': [],
    'sfm_ndwarp_o2d2.hip': _NDWARP,
    'sfm_mfma_g6x7.hip': _MFMA,
    'sfm_mfma_g8x9.hip': _MFMA,
    'sfm_mfma_g7x8.hip': _MFMA,
    'sfm_mesh.hip': ['-ffp-contract=off'] + os.environ.get('SFM_MESH_FLAGS', '').split(),  # 10 s
    'sfm_mfma_g5x6.hip': _MFMA,
    'sfm_mfma_g4x5.hip': _MFMA,
    'sfm_mfma_g3x4.hip': _MFMA,
    'sfm_ndwarp_o5d3_image.hip': _NDWARP,
    'sfm_ndwarp_o4d3_image.hip': _NDWARP,
    'sfm_mfma_g20x11.hip': _MFMA,
    'sfm_mfma_g15x11.hip': _MFMA,
    'sfm_xcorr_mfma.hip': _MFMA,             # 5 s
    'sfm_fft_own.hip': [],
    'sfm_spline.hip': ['-ffp-contract=off'],
    'sfm_invmap.hip': ['-ffp-contract=off'],
    'sfm_maps.hip': ['-ffp-contract=off'] + os.environ.get('SFM_MAPS_FLAGS', '').split(),
    'sfm_mapgeom.hip': ['-ffp-contract=off'],
    'sfm_core.hip': [],
    'sfm_flowutils.hip': ['-ffp-contract=off'],
    'sfm_fillmissing.hip': [],
    'sfm_comm.hip': [],
    'sfm_xcorr_fft.hip': [],
    'sfm_mfma_host.hip': _MFMA,
    'sfm_tileflows.hip': ['-ffp-contract=off'],
    'sfm_warp.hip': ['-ffp-contract=off'],   # 2 s
}
# SFM_BUILD_FLAGS: extra flags for every unit (-DSFM_MEASUREMENT_SWITCHES: the library
# honours the measurement-only switches, see csrc/sfm_common.h)
COMMON = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC',
          '-Wno-unused-result'] + os.environ.get('SFM_BUILD_FLAGS', '').split()


def _hipcc() -> str:
  exe = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
  if not os.path.exists(exe):
    raise RuntimeError('hipcc not found; cannot build libsofima_amd.so')
  return exe


def _stale(target: str, deps: list[str], cmd: list[str] | None = None) -> bool:
  """Out of date by mtime, or built with a different command line (the extra
  flags come from environment variables: an instrumented build must not
  silently stay the production library, nor the reverse)."""
  if not os.path.exists(target):
    return True
  t = os.path.getmtime(target)
  if any(os.path.getmtime(d) > t for d in deps):
    return True
  if cmd is not None:
    try:
      with open(target + '.cmd') as f:
        return f.read() != ' '.join(cmd)
    except OSError:
      return True
  return False


def _record(target: str, cmd: list[str]) -> None:
  with open(target + '.cmd', 'w') as f:
    f.write(' '.join(cmd))


def jobs() -> int:
  """Compiler processes at a time: MAX_JOBS if set, else the CPU count; 1 .. 16."""
  try:
    n = int(os.environ.get('MAX_JOBS', ''))
  except ValueError:
    n = os.cpu_count() or 1
  return max(1, min(n, 16))


def _compile(cmd: list[str], obj: str) -> subprocess.CompletedProcess:
  # (a unit that fails must not leave an object that looks fresh)
  for path in (obj, obj + '.cmd'):
    if os.path.exists(path):
      os.remove(path)
  done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
  if done.returncode == 0:
    _record(obj, cmd)
  return done


def build(force: bool = False, verbose: bool = False) -> str:
  """Compiles every HIP translation unit for gfx950, the stale ones side by side,
  and links the library."""
  os.makedirs(LIB_DIR, exist_ok=True)
  os.makedirs(OBJ_DIR, exist_ok=True)
  headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC)
             if f.endswith('.h')]
  headers.append(os.path.join(PKG_DIR, '..', 'include', 'sofima_amd.h'))
  hipcc = _hipcc()
  objs = []
  stale = []
  for src, extra in SOURCES.items():
    src_path = os.path.join(CSRC, src)
    obj = os.path.join(OBJ_DIR, src + '.o')
    objs.append(obj)
    cmd = [hipcc] + COMMON + extra + ['-c', src_path, '-o', obj]
    if force or _stale(obj, [src_path] + headers, cmd):
      if verbose:
        print(' '.join(cmd))
      stale.append((src, cmd, obj))
  with ThreadPoolExecutor(max_workers=jobs()) as pool:
    results = list(pool.map(lambda job: _compile(job[1], job[2]), stale))
  for (src, _, _), done in zip(stale, results):
    if done.returncode != 0:
      # (the library, if any, is older than the source that failed: still stale)
      raise RuntimeError('%s failed to compile:\n%s' % (src, done.stdout))
    if done.stdout:   # warnings
      print(done.stdout, end='')
  if stale or _stale(LIB_PATH, objs):
    # no library dependency beyond the HIP runtime (RCCL is resolved with dlsym)
    cmd = [hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB_PATH
           ] + objs + ['-L/opt/rocm/lib', '-ldl', '-Wl,-rpath,/opt/rocm/lib']
    if verbose:
      print(' '.join(cmd))
    subprocess.run(cmd, check=True)
    _stamp()
  return LIB_PATH


def source_hash() -> str:
  """Hash of the kernel sources (csrc/ + the C header): names the BUILD that
  measurements belong to.  Unlike a git revision it survives documentation
  commits and rebuilds of unchanged sources."""
  import hashlib
  h = hashlib.sha256()
  files = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC)
                 if f.endswith(('.hip', '.h')))
  files.append(os.path.join(PKG_DIR, '..', 'include', 'sofima_amd.h'))
  for path in files:
    h.update(os.path.basename(path).encode())
    with open(path, 'rb') as f:
      h.update(f.read())
  return h.hexdigest()[:12]


def _stamp() -> None:
  """Records the source hash the library was linked from (.build_sha, not
  tracked): the profile scripts stamp their counter summaries with it.  The
  snapshot a GPU box receives has no .git, so the file travels with the .so."""
  try:
    with open(os.path.join(PKG_DIR, '..', '.build_sha'), 'w') as f:
      f.write(source_hash() + '\n')
  except OSError:
    pass


if __name__ == '__main__':
  print(build(force=False, verbose=True))
