#!/bin/bash
# Development aid: links libtactile_gym_hip.so from the objects already in ../lib (after compiling single translation units by hand) and marks
# every object fresh for build.sh's TG_INCREMENTAL rule.  The build of record is build.sh; HIPCC, TG_OUT and TG_DRY_RUN mean what they mean there.
set -euo pipefail
cd "$(dirname "$0")"
. ./units.sh
link libtactile_gym_hip.so "${PRODUCT_OBJS[@]}"
[ "$DRY" = "1" ] || { touch "$OUT"/*.o; ls -la "$OUT/libtactile_gym_hip.so"; }
