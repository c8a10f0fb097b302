"""The relaxation driver of a section: regular / prepared / regularised passes.

Drop-in for the compute part of `processor/mesh.py: RelaxMesh.relax_mesh`
(processor/mesh.py:428-513), the step right after the hot path (SURVEY.md 8f,
rank 4): relax; if `map_utils.mask_irregular` finds folds, relax a fresh mesh
towards the first solution with k0 / 10, and if that one is regular, relax it
again against the real targets.  All three relaxations and both fold tests run
on the device; the mesh state stays in HBM between them and goes to the host
once, at the end.

`prev_state` is the function that feeds that solver: `RelaxMesh.get_prev_state`
with `compute_ref_mesh` and `compute_ref_mesh_multiz` (processor/mesh.py:170-385).
A section is aligned against several earlier sections at once, through
2-channel flows of a fixed look-back and 3-channel flows whose third channel
names the look-back per node; every flow is composed with the solved mesh it
points at, the results are averaged per node in float64 and fold-masked, all in
two device calls.  `relax_sections` is the loop a caller of
`RelaxMesh.run_relaxation` (:515-552) runs section by section, with the solved
meshes kept in HBM.

The chunking / volume I/O of the `RelaxMesh` processor (connectomics
subvolumes, TensorStore) stays out of scope; it calls these functions where it
called its methods.
"""
from __future__ import annotations

import bisect
import ctypes as C
import dataclasses
import enum
import logging
from typing import Any, Sequence

import numpy as np

from . import flow_utils
from . import map_utils
from . import mesh as mesh_lib


class SolutionStatus(enum.IntEnum):
  """processor/mesh.py:41-45."""
  UNDEFINED = -1
  REGULAR = 0
  PREP_FAILED = 1
  REGULARIZED = 2


class MeshInitState(enum.Enum):
  """processor/mesh.py:48-50."""
  ZEROS = 0
  PREV_MEDIAN = 1


def maybe_update_init_state(x: np.ndarray, prev: np.ndarray | None,
                            init_state: MeshInitState = MeshInitState.ZEROS
                            ) -> np.ndarray:
  """processor/mesh.py:387-398: optionally start from the median offset of the
  reference section."""
  if init_state == MeshInitState.PREV_MEDIAN and prev is not None:
    prev = np.asarray(prev)
    x[0, ...] = np.nanmedian(prev[0, ...])
    x[1, ...] = np.nanmedian(prev[1, ...])
    x = np.nan_to_num(x)
  return x


def relax_mesh(x: np.ndarray, prev: np.ndarray,
               integration_config: mesh_lib.IntegrationConfig,
               mask: np.ndarray | None = None, mesh_min_frac: float = 0.5,
               init_state: MeshInitState = MeshInitState.ZEROS
               ) -> tuple[np.ndarray, list[float], int, SolutionStatus]:
  """Performs mesh relaxation with the fold-recovery passes
  (processor/mesh.py:428-513).

  x, prev: [2, 1, y, x]; mask: optional [1, y, x] boolean, True entries of x
  are set to NaN (in place, like the reference).  Returns (optimised positions
  [np.ndarray], kinetic-energy history, steps simulated, SolutionStatus).

  `prev` may be a DeviceArray of an earlier call.  Like the reference,
  `mask_irregular` works IN PLACE on the solution it tests (map_utils.py:737-786
  modifies its argument, a view of x); PREP_FAILED returns the copy taken
  before the first test.
  """
  x_t, e_kin, num_steps, status = _relax_mesh_device(x, prev, integration_config, mask,
                                                      mesh_min_frac, init_state)
  return x_t.cpu().numpy(), e_kin, num_steps, status


def _relax_mesh_device(x, prev, integration_config, mask, mesh_min_frac, init_state):
  """relax_mesh with the solution left on the device (a float32 tensor)."""
  from . import _dev
  if mask is not None:
    flow_utils.apply_mask(x, mask)
  logging.info('Starting mesh relaxation.')
  dev = _dev.device()
  prev_d = _dev.as_device_f32(prev, dev, copy=False)      # uploaded once
  stride = integration_config.stride
  x_d, e_kin, num_steps = mesh_lib.relax_mesh(x, prev_d, integration_config)
  orig_x = x_d.tensor.clone()
  # the fold test NaNs the irregular nodes of the solution in place, on the device
  masked = map_utils.mask_irregular(x_d.tensor[:, 0], stride, mesh_min_frac,
                                    dilation_iters=5)
  if not np.any(masked):
    return x_d.tensor, e_kin, num_steps, SolutionStatus.REGULAR

  logging.info('Attempting relaxation with 10% k0.')
  # A new initial state that is similar to the previous solution everywhere
  # except near the irregular nodes; if it relaxes to a regular mesh, simulate
  # again from there, otherwise return the original solution.
  start_x = maybe_update_init_state(np.zeros(x_d.shape, np.float32), prev, init_state)
  x_d, _, prep_steps = mesh_lib.relax_mesh(
      start_x, x_d,
      dataclasses.replace(integration_config, k0=integration_config.k0 / 10.0))
  masked = map_utils.mask_irregular(x_d.tensor[:, 0], stride, mesh_min_frac)
  if np.any(masked):
    return (orig_x, e_kin, num_steps + prep_steps,
            SolutionStatus.PREP_FAILED)

  if mask is not None:
    m = _dev.as_device_mask(mask, dev).bool()
    x_d.tensor[:, m] = float('nan')
  x_d, e_kin2, reg_steps = mesh_lib.relax_mesh(x_d, prev_d, integration_config)
  return (x_d.tensor, e_kin2, num_steps + prep_steps + reg_steps,
          SolutionStatus.REGULARIZED)


class FlowVolume:
  """An inter-section flow volume (processor/mesh.py:53-58): `flow` is
  [2 or 3, nz, y, x] (NumPy, torch or DeviceArray), `delta_z` the look-back it
  was computed with (negative when solving backward).  The channel count plays
  the role of the reference's `meta.num_channels`: a third channel holds, per
  node, how many sections back the vector was measured."""

  def __init__(self, flow: Any, delta_z: int):
    shape = tuple(np.shape(flow))
    if len(shape) != 4 or shape[0] not in (2, 3):
      raise ValueError('flow must be [2 or 3, nz, y, x]')
    self.flow = flow
    self.delta_z = int(delta_z)
    self.shape = shape
    self._device = None

  @property
  def num_channels(self) -> int:
    return self.shape[0]

  def device_tensor(self, dev):
    """The flow as a float32 device tensor, uploaded once."""
    from . import _dev
    if self._device is None:
      self._device = _dev.as_device_f32(self.flow, dev, copy=False)
    return self._device

  def lookbacks(self, z: int) -> list[int]:
    """The look-back offsets named by channel 2 of section z: the distinct
    values that are whole numbers other than 0, nearest first
    (processor/mesh.py:181-188)."""
    import torch
    from . import _dev
    plane = self.flow.tensor if isinstance(self.flow, _dev.DeviceArray) else self.flow
    if isinstance(plane, torch.Tensor):
      vals = torch.unique(plane[2, z]).cpu().numpy()
    else:
      vals = np.unique(np.asarray(plane[2, z]))
    vals = vals[np.isfinite(vals) & (vals != 0)]
    vals = vals[(vals == np.trunc(vals)) & (np.abs(vals) < 2.0**31)]
    return sorted((int(v) for v in vals), key=abs)


def _block_id(z: int, starts: Sequence[int], backward: bool) -> int:
  """client_utils.get_block_id."""
  return bisect.bisect_left(starts, z) if backward else bisect.bisect_right(starts, z)


def _plan_section(z, flows, block_starts, backward, sections_to_skip):
  """[(flow index, [ref z, ...]), ...] of the flows that take part in the
  reference positions of section z, or None where get_prev_state returns None
  (processor/mesh.py:296-367).  A 3-channel flow whose offsets all leave the
  block still takes part, with no reference."""
  starts = sorted(int(s) for s in block_starts)
  if z in starts:
    return None
  skip = set(int(s) for s in sections_to_skip)
  curr_block = _block_id(z, starts, backward)
  plan = []
  for i, fv in enumerate(flows):
    ref_z = z - fv.delta_z
    if ref_z in skip:                       # do not align to skipped sections
      continue
    if _block_id(ref_z, starts, backward) != curr_block:
      continue
    if fv.num_channels == 2:
      plan.append((i, [ref_z]))
      continue
    refs = []
    for dz in fv.lookbacks(z):              # nearest first; the first one that
      if _block_id(z - dz, starts, backward) != curr_block:   # leaves the block ends
        break                               # the search (ignore_xblock=True)
      refs.append(z - dz)
    plan.append((i, refs))
  return plan or None


def refs_for_section(z: int, flows: Sequence[FlowVolume], block_starts: Sequence[int],
                     backward: bool = False, sections_to_skip: Sequence[int] = ()
                     ) -> list[tuple[int, int]] | None:
  """The (flow index, reference z) pairs `RelaxMesh.get_prev_state` loads a
  solved mesh for when it builds the reference positions of section z, in its
  order; None where it returns None (a block start, or no flow takes part).

  Every flow is tried with its own `delta_z` first: a flow whose section
  z - delta_z is skipped or lies in another block (`client_utils.get_block_id`:
  bisect_right, or bisect_left when backward) is left out as a whole.  A
  2-channel flow then refers to that one section.  A 3-channel flow refers to
  z - dz for the look-backs dz of its third channel, nearest first, up to the
  first one that leaves the block; these are not checked against
  `sections_to_skip`, as in the reference.  Host logic only.
  """
  plan = _plan_section(z, flows, block_starts, backward, sections_to_skip)
  if plan is None:
    return None
  return [(i, rz) for i, refs in plan for rz in refs]


def _device_planes(x, dev, n):
  """x: [c, y, x] -> (float32 device tensor, channel stride in elements).  A
  device view whose [y, x] planes are dense and do not overlap is taken where it
  lies (a section of a [c, nz, y, x] volume: channel stride nz * y * x); anything
  else is copied once."""
  import torch
  from . import _dev
  t = x.tensor if isinstance(x, _dev.DeviceArray) else x
  if isinstance(t, torch.Tensor):
    t = t.to(device=dev, dtype=torch.float32)
  else:
    t = _dev.as_device_f32(t, dev, copy=False)
  if t.ndim == 3 and (t.stride(2) != 1 or t.stride(1) != t.shape[2] or
                      (t.shape[0] > 1 and t.stride(0) < n)):
    t = t.contiguous()
  return t, (t.stride(0) if t.ndim == 3 and t.shape[0] > 1 else n)


def _prev_state_desc(flows, refs, stride, dev):
  """(SfmPrevStateDesc, the tensors it points into, (y, x)) of compose_average."""
  from . import _abi, _dev
  if not 1 <= len(flows) <= _abi.PREV_MAX_FLOWS or len(refs) != len(flows):
    raise ValueError(f'1 to {_abi.PREV_MAX_FLOWS} flows, one reference table each')
  d = _abi.SfmPrevStateDesc()
  keep = []
  shape = tuple(np.shape(flows[0])[1:])
  if len(shape) != 2:
    raise ValueError('flows must be [2 or 3, y, x] of one shape')
  n = shape[0] * shape[1]
  for f, (flow, table) in enumerate(zip(flows, refs)):
    t, cs = _device_planes(flow, dev, n)
    if t.ndim != 3 or t.shape[0] not in (2, 3) or tuple(t.shape[1:]) != shape:
      raise ValueError('flows must be [2 or 3, y, x] of one shape')
    if len(table) > _abi.PREV_MAX_REFS or (t.shape[0] == 2 and len(table) != 1):
      raise ValueError('one reference per 2-channel flow, at most '
                       f'{_abi.PREV_MAX_REFS} per 3-channel flow')
    keep.append(t)
    fl = d.flows[f]
    fl.channels = t.shape[0]
    fl.n_refs = len(table)
    fl.flow = t.data_ptr()
    fl.flow_channel_stride = cs
    mesh_cs = None
    for k, (dz, mesh) in enumerate(table):
      if tuple(np.shape(mesh)) != (2,) + shape:
        raise ValueError('a reference mesh must be [2, y, x] of the flows\' shape')
      m, mcs = _device_planes(mesh, dev, n)
      if mesh_cs is not None and mcs != mesh_cs:
        m = m.contiguous()                  # one plane stride per flow
        mcs = n
        if mcs != mesh_cs:
          raise ValueError('reference meshes of one flow must share their plane stride')
      mesh_cs = mcs
      keep.append(m)
      fl.delta_z[k] = int(dz)
      fl.mesh[k] = m.data_ptr()
    fl.mesh_channel_stride = mesh_cs if mesh_cs is not None else n
  d.shape = (C.c_int32 * 2)(*shape)
  d.n_flows = len(flows)
  sy, sx = (float(v) for v in (stride if np.ndim(stride) else (stride, stride)))
  d.stride = (C.c_float * 2)(sy, sx)
  d.stream = _dev.stream_ptr()
  return d, keep, shape


def compose_average(flows: Sequence[Any], refs: Sequence[Sequence[tuple[int, Any]]],
                    stride: Sequence[float]):
  """The fused "compose and average" call (sfm_prev_state) for one section.

  flows: up to 8 arrays [2 or 3, y, x]; refs: per flow the (look-back dz, solved
  mesh [2, y, x] of section z - dz) entries, exactly one for a 2-channel flow,
  up to 16 for a 3-channel flow; stride: as handed to `compose_maps_fast`.
  Float32 device views with dense [y, x] planes (sections of [c, nz, y, x]
  volumes) are read in place.  Returns the float64 [2, y, x] per-node mean on
  the device (a torch tensor).
  """
  import torch
  from . import _abi, _dev
  dev = _dev.device()
  d, keep, shape = _prev_state_desc(flows, refs, stride, dev)
  out = torch.empty((2,) + shape, dtype=torch.float64, device=dev)
  _abi.check(_abi.load().sfm_prev_state(C.byref(d), out.data_ptr()))
  del keep
  return out


def _prev_state_device(z, flows, history, stride, plan, masked_history, mesh_min_frac,
                       mesh_max_frac, irregular_mask_radius):
  """(prev [2, y, x] float64 tensor, n_valid device int) of a planned section."""
  from . import _dev
  dev = _dev.device()
  planes, tables = [], []
  for i, ref_zs in plan:
    fv = flows[i]
    planes.append(fv.device_tensor(dev)[:, z])
    if fv.num_channels == 2:
      # the reference masks this path only when it was given an initial mesh
      # volume (processor/mesh.py:262-264), which is out of scope here
      tables.append([(fv.delta_z, history[:, ref_zs[0]])])
    else:
      src = history if masked_history is None else masked_history
      tables.append([(z - rz, src[:, rz]) for rz in ref_zs])
  prev = compose_average(planes, tables, stride)
  _, n_valid = map_utils.mask_irregular_f64(prev, stride, mesh_min_frac, mesh_max_frac,
                                            dilation_iters=irregular_mask_radius)
  return prev, n_valid


def prev_state(z: int, flows: Sequence[FlowVolume], history, stride: Sequence[float], *,
               block_starts: Sequence[int], backward: bool = False,
               sections_to_skip: Sequence[int] = (), masked_history=None,
               mesh_min_frac: float, mesh_max_frac: float,
               irregular_mask_radius: int = 1):
  """Positions of the reference nodes of section z (`RelaxMesh.get_prev_state`,
  processor/mesh.py:279-385): a [2, 1, y, x] float64 DeviceArray, or None for a
  block start and for a section no flow takes part in.

  history: [2, nz, y, x] float32 solved meshes (device tensor, DeviceArray or
  NumPy); the sections `refs_for_section` names must be solved.
  masked_history: the same with the invalid-tissue nodes of every section set
  to NaN; when given, 3-channel flows are composed with it (:213-215).  Flows
  measured against more than one section are averaged with per-node counts in
  float64, then `mask_irregular` runs on the float64 average with
  `mesh_min_frac`, `mesh_max_frac` and `irregular_mask_radius` dilations.
  """
  from . import _dev
  plan = _plan_section(z, flows, block_starts, backward, sections_to_skip)
  if plan is None:
    return None
  dev = _dev.device()
  history = _dev.as_device_f32(history, dev, copy=False)
  if masked_history is not None:
    masked_history = _dev.as_device_f32(masked_history, dev, copy=False)
  prev, _ = _prev_state_device(z, flows, history, stride, plan, masked_history, mesh_min_frac,
                               mesh_max_frac, irregular_mask_radius)
  return _dev.DeviceArray(prev[:, None])


def relax_sections(flows: Sequence[FlowVolume],
                   integration_config: mesh_lib.IntegrationConfig, *,
                   block_starts: Sequence[int], backward: bool = False,
                   sections_to_skip: Sequence[int] = (), mask=None,
                   mesh_min_frac: float, mesh_max_frac: float,
                   init_state: MeshInitState = MeshInitState.ZEROS,
                   irregular_mask_radius: int = 1, solved=None,
                   sections: Sequence[int] | None = None
                   ) -> tuple[np.ndarray, list[SolutionStatus], list[int], list[list[float]]]:
  """Solves the sections of a volume one after the other, each against the
  solved sections before it: the loop a caller of `RelaxMesh.run_relaxation`
  (processor/mesh.py:515-552) runs, for a configuration without an initial
  mesh volume.

  flows: FlowVolumes of one [nz, y, x] extent.  mask: optional [nz, y, x]
  boolean, True = invalid tissue; the nodes are removed from the section being
  solved, and from the reference meshes of 3-channel flows (the reference's
  2-channel path masks only when it has an initial mesh volume; that quirk is
  kept).  solved: optional [2, nz, y, x] meshes of sections solved earlier (the
  reference reads them back from its output volume).  sections: the z to solve
  now, in solve order; default all, descending when `backward`.  The first one
  must be a block start.

  A block start, and a section whose reference positions are None or all NaN,
  keeps the zero mesh with status UNDEFINED and 0 steps; any other section is
  `relax_mesh(zeros, prev, ...)`.  The solved meshes stay on the device between
  sections.  Returns (meshes [2, nz, y, x] float32, statuses [nz], steps [nz],
  kinetic-energy histories [nz]), what `run_relaxation` returns per section;
  sections not solved in this call keep what `solved` gave them and report
  UNDEFINED / 0 / [].

  Not covered, and not parameters: `coming_in` regions, `ranges_to_skip` with
  their custom flow volumes, an initial `mesh` volume and volume I/O.
  `EstimateMissingFlow` itself, which produces the 3-channel flows, is
  `processor_flow.estimate_missing_flow`.
  """
  if not flows:
    raise ValueError('no flows')
  nz, ny, nx = flows[0].shape[1:]
  if any(fv.shape[1:] != (nz, ny, nx) for fv in flows):
    raise ValueError('flows must share their [nz, y, x] extent')
  starts = sorted(int(s) for s in block_starts)
  if sections is None:
    sections = range(nz - 1, -1, -1) if backward else range(nz)
  sections = [int(z) for z in sections]
  if any(not 0 <= z < nz for z in sections):
    raise ValueError('section out of range')
  if sections and sections[0] not in starts:
    raise ValueError(f'the first section to solve ({sections[0]}) must be a block start')
  mask_h = None
  if mask is not None:
    mask_h = np.asarray(mask).astype(bool)
    if mask_h.shape != (nz, ny, nx):
      raise ValueError('mask must be [nz, y, x]')

  import torch
  from . import _dev
  dev = _dev.device()
  history = torch.zeros((2, nz, ny, nx), dtype=torch.float32, device=dev)
  if solved is not None:
    history.copy_(_dev.as_device_f32(solved, dev, copy=False))
  masked_history = mask_d = None
  if mask_h is not None:
    # masking has to reach the bilinear taps: a second, masked plane per section
    mask_d = _dev.as_device_mask(mask_h, dev).bool()
    masked_history = history.clone()
    masked_history[:, mask_d] = float('nan')
  statuses = [SolutionStatus.UNDEFINED] * nz
  steps = [0] * nz
  energies = [[] for _ in range(nz)]
  stride = integration_config.stride
  for z in sections:
    history[:, z] = 0
    plan = _plan_section(z, flows, starts, backward, sections_to_skip)
    if plan is not None:
      prev, n_valid = _prev_state_device(z, flows, history, stride, plan, masked_history,
                                         mesh_min_frac, mesh_max_frac, irregular_mask_radius)
      if int(n_valid.item()) > 0:        # not np.all(np.isnan(prev))
        x_t, energies[z], steps[z], statuses[z] = _relax_mesh_device(
            np.zeros((2, 1, ny, nx), np.float32), _dev.DeviceArray(prev[:, None]),
            integration_config, None if mask_h is None else mask_h[z:z + 1], mesh_min_frac,
            init_state)
        history[:, z] = x_t[:, 0]
    if masked_history is not None:
      masked_history[:, z] = history[:, z]
      masked_history[:, z][:, mask_d[z]] = float('nan')
  return history.cpu().numpy(), statuses, steps, energies
