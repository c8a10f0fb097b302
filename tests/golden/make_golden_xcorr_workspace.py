"""Generates tests/golden/xcorr_workspace.json: what sfm_xcorr_workspace_bytes
returns, and the message behind every refusal, for a table of descriptors that
covers every correlation path and every way a call is split into rounds.

Run ONCE against the library whose sizes are the record (the commit before the
correlation driver got its single plan), never by the test:
  python -m sofima_amd._build          # of that commit
  python tests/golden/make_golden_xcorr_workspace.py
It needs no GPU.  `path` is not read by the library: it names the path the case was
chosen to land on, for the coverage check of the test.
"""
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from sofima_amd import _abi  # noqa: E402

PRE, POST, STARTS = 0x10000, 0x20000, 0x30000   # eligibility reads `image & 3`
DTYPES = {'u8': _abi.DTYPE_U8, 'f32': _abi.DTYPE_F32}


def make_desc(case):
  """The descriptor of one fixture case (None: the NULL descriptor)."""
  if case.get('null'):
    return None
  i3 = lambda v: (C.c_int32 * 3)(*([1] * (3 - len(v)) + list(v)))
  d = _abi.SfmXcorrDesc()
  d.ndim = case['ndim']
  d.dtype = DTYPES[case['dtype']]
  d.pre_image = PRE + case.get('misalign', 0)
  d.post_image = POST
  d.pre_shape = d.post_shape = i3(case['image'])
  if case['masked']:
    d.pre_mask, d.post_mask = PRE + 0x8000, POST + 0x8000
    d.pre_mask_shape = d.post_mask_shape = i3(case['image'])
  d.patch = i3(case['patch'])
  d.post_patch = i3(case['post_patch'])
  d.pre_starts = d.post_starts = STARTS
  d.batch, d.group = case['batch'], case['group']
  d.use_mean = 0
  d.min_distance, d.threshold_rel = 2, 0.5
  d.peak_radius = i3([5] * case['ndim'])
  d.method = case['method']
  return d


def measure(case):
  """(bytes, message or None) of one case, under the case's option switches."""
  lib = _abi.load()
  d = make_desc(case)
  switches = [_abi.option(k, v) for k, v in case.get('options', {}).items()]
  for s in switches:
    s.__enter__()
  try:
    n = lib.sfm_xcorr_workspace_bytes(None if d is None else C.byref(d))
  finally:
    for s in reversed(switches):
      s.__exit__(None, None, None)
  return n, (None if n else lib.sfm_last_error().decode())


AUTO, DIRECT, MFMA_I8, FFT = 0, 1, 2, 3
U8_48 = dict(ndim=2, dtype='u8', image=[240, 280], patch=[48, 48], post_patch=[48, 48])
F32_24 = dict(ndim=2, dtype='f32', image=[240, 280], patch=[24, 24], post_patch=[24, 20])
F32_3D = dict(ndim=3, dtype='f32', image=[20, 40, 40], patch=[8, 12, 12],
              post_patch=[8, 12, 12])
F32_300 = dict(ndim=2, dtype='f32', image=[400, 400], patch=[300, 300],
               post_patch=[300, 300])


def case(name, path, geo, batch, group, method, masked, **extra):
  return dict(name=name, path=path, **geo, batch=batch, group=group, method=method,
              masked=masked, **extra)


CASES = [
    case('mfma_ragged', 'mfma', U8_48, 11, 4, AUTO, False),
    case('mfma_one_group', 'mfma', U8_48, 8, 8, MFMA_I8, False),
    case('mfma_masked_ragged', 'mfma_masked', U8_48, 11, 4, AUTO, True),
    case('mfma_masked_one_group', 'mfma_masked', U8_48, 8, 0, AUTO, True),
    # 10 groups: more than one round of SFM_MASKED_GROUPS (8) groups
    case('mfma_masked_rounds', 'mfma_masked', U8_48, 40, 4, AUTO, True),
    case('mfma_masked_rounds_of_2', 'mfma_masked', U8_48, 40, 4, AUTO, True,
         options={'SFM_MASKED_GROUPS': 2}),
    case('u8_direct_ragged', 'direct', U8_48, 11, 4, DIRECT, False),
    case('u8_misaligned_is_not_mfma', 'fft', U8_48, 11, 4, AUTO, False, misalign=1),
    case('direct_masked_ragged', 'direct', F32_24, 11, 4, AUTO, True),
    case('direct_group_0', 'direct', F32_24, 11, 0, DIRECT, False),
    case('direct_group_above_batch', 'direct', F32_24, 11, 16, DIRECT, False),
    case('direct_ragged', 'direct', F32_24, 11, 4, AUTO, False),
    case('fft_ragged', 'fft', F32_24, 11, 4, FFT, False),
    case('fft_masked_ragged', 'fft', F32_24, 11, 4, FFT, True),
    case('fft_one_group', 'fft', F32_24, 8, 8, FFT, False),
    case('fft_auto_large_patch', 'fft', dict(F32_24, patch=[48, 48], post_patch=[48, 48]),
         11, 4, AUTO, False),
    case('fft_3d', 'fft', F32_3D, 5, 2, FFT, False),
    case('direct_3d_masked', 'direct', F32_3D, 5, 2, DIRECT, True),
    case('direct_gather_partials', 'direct', F32_300, 3, 2, DIRECT, False),
    case('fft_gather_partials_masked', 'fft', F32_300, 3, 2, AUTO, True),
    # refusals: 0 bytes and a message
    dict(name='null_descriptor', null=True),
    case('batch_0', None, F32_24, 0, 0, AUTO, False),
    case('mfma_on_float', None, F32_24, 11, 4, MFMA_I8, False),
    case('fft_volume_beyond_transforms', None,
         dict(ndim=3, dtype='f32', image=[1000, 8, 8], patch=[1000, 8, 8],
              post_patch=[1000, 8, 8]), 1, 1, FFT, False),
]


def main():
  for c in CASES:
    c['bytes'], c['error'] = measure(c)
    print(c['name'], c['bytes'], c['error'])
  with open(os.path.join(HERE, 'xcorr_workspace.json'), 'w') as f:
    json.dump({'cases': CASES}, f, indent=1)
    f.write('\n')


if __name__ == '__main__':
  main()
