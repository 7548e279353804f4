#!/bin/bash
# A variant of the RELEASE library whose fused member kernel (greb_member.hip) is compiled with other flags:
#   tools/build_member_variant.sh <tag> <flags...>  ->  variants/libgreb_member_<tag>.so  (GREB_BENCH_LIB=... bench.py)
tag=$1; shift
cd "$(dirname "$0")/.." && exec python -m greb_climate_model_amd.build variant "member_$tag" release greb_member.hip "$@"
