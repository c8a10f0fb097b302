#!/bin/bash
# Measurement build of the library beside the production one:
#   sofima_amd/lib/libsofima_amd_timing.so   (select it with SOFIMA_AMD_LIB=...)
# = the units of the matrix-core correlation path with clock64 phase ticks + device printf
# (-DSFM_MFMA_TIMING) and the
# measurement-only switches (-DSFM_MEASUREMENT_SWITCHES: SFM_MFMA_PROBE / TOUCH_ALL / EXACT /
# QUEUE / PRIO / MAX_WG_PER_CU / GUARD_2R, which the production library ignores).  Built here, on the CPU
# box -- it travels with gpurun.  NOTIMING=1: the switches without the ticks
# (libsofima_amd_measure.so: production timing behaviour, for A/B runs and the identity tests
# of those switches).
set -e
R=$(cd "$(dirname "$0")/../.." && pwd)
python -c "from sofima_amd import _build; _build.build()"
O=$R/sofima_amd/build
T=-DSFM_MFMA_TIMING; NAME=timing
if [ -n "$NOTIMING" ]; then T=; NAME=measure; fi
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-result -DSFM_MEASUREMENT_SWITCHES"
# (the units of the matrix-core path are _build.MFMA_UNITS; sfm_core.hip answers for the switches)
MFMA=$(python -c "from sofima_amd import _build; print(' '.join(_build.MFMA_UNITS))")
JOBS=$(python -c "from sofima_amd import _build; print(_build.jobs())")
{ for u in $MFMA; do echo "$T $SFM_MFMA_FLAGS -c $R/sofima_amd/csrc/$u -o $O/${u%.hip}_$NAME.o"; done
  echo "-c $R/sofima_amd/csrc/sfm_core.hip -o $O/sfm_core_$NAME.o"; } | xargs -P $JOBS -L 1 hipcc $F
OBJS=$(python -c "from sofima_amd import _build; print(' '.join('$O/%s.o' % u for u in _build.SOURCES if u not in _build.MFMA_UNITS + ('sfm_core.hip',)))")
NEW=$(for u in $MFMA sfm_core.hip; do echo $O/${u%.hip}_$NAME.o; done)
hipcc --offload-arch=gfx950 -shared -fPIC -o $R/sofima_amd/lib/libsofima_amd_$NAME.so \
  $OBJS $NEW -L/opt/rocm/lib -ldl -Wl,-rpath,/opt/rocm/lib
ls -la $R/sofima_amd/lib/
