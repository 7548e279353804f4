#!/bin/bash
# A variant of the tuning library whose row-strip kernels are compiled with extra -D flags, for A/B runs of compile-time choices:
#   tools/build_variant.sh <tag> -DGREB_ROWS_SLOTS=6 ...   ->  variants/libgreb_<tag>.so   (GREB_LIB=... selects it)
tag=$1; shift
cd "$(dirname "$0")/.." && exec python -m greb_climate_model_amd.build variant "$tag" tuning greb_rows.hip,greb_step_rows.hip "$@"
