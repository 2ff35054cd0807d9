#!/bin/bash
# Builds libtactile_gym_hip.so (the product) and libtactile_gym_hip_test.so (device self-tests over the product's own objects, declared in
# include/tactile_gym_hip_test.h and loaded by tests/ only) for gfx950 (MI355X) in-tree.  hipcc cross-compiles without a GPU.
# units.txt names every translation unit, its library and its flags, and says why; the order of its lines is the start and the link order.
#   HIPCC            the compiler driver (default /opt/rocm/bin/hipcc)
#   TG_OUT           another output directory (audit / A-B builds: TG_EXTRA_FLAGS=... TG_OUT=../lib_audit, loaded with TG_HIP_LIBRARY)
#   TG_EXTRA_FLAGS   appended to every compile command
#   TG_INCREMENTAL=1 (development) keep an object whose translation unit and every header are older than it
#   TG_JOBS          compilers running at a time (default: MAX_JOBS if set, else the CPUs of the machine, at most 16)
#   TG_DRY_RUN=1     print the job limit, every compile command and both link commands, one per line; run nothing
set -euo pipefail
cd "$(dirname "$0")"
. ./units.sh
COMMON="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value ${TG_EXTRA_FLAGS:-}"
cpus=$(nproc)
JOBS=${TG_JOBS:-${MAX_JOBS:-$((cpus < 16 ? cpus : 16))}}
[[ $JOBS =~ ^[1-9][0-9]*$ ]] || { echo "build.sh: TG_JOBS (or MAX_JOBS) must be a positive number, not '$JOBS'" >&2; exit 2; }
if [ "$DRY" = "1" ]; then echo "# at most $JOBS compilers at a time"; else mkdir -p "$OUT"; fi
stale() {   # stale <object> <source>: 0 if the object must be rebuilt
    [ "${TG_INCREMENTAL:-0}" = "1" ] || return 0
    [ -f "$1" ] || return 0
    for f in "$2" *.hpp *.h ../../include/*.h; do [ "$f" -nt "$1" ] && return 0; done
    return 1
}
cc() {      # cc <name> <extra flags...>
    local name=$1; shift
    if stale "$OUT/$name.o" "$name.hip"; then
        [ "$DRY" = "1" ] || rm -f "$OUT/$name.o"
        run $HIPCC $COMMON "$@" -c "$name.hip" -o "$OUT/$name.o"
    fi
}
running=0; failed=0
reap() {    # one finished compiler: the first failure's exit status is the build's
    local rc=0; wait -n || rc=$?
    running=$((running - 1)); [ "$failed" -ne 0 ] || failed=$rc
}
for i in "${!UNITS[@]}"; do
    [ "$running" -lt "$JOBS" ] || reap
    [ "$failed" -eq 0 ] || break
    cc "${UNITS[$i]}" ${UNIT_FLAGS[$i]} &
    running=$((running + 1))
done
while [ "$running" -gt 0 ]; do reap; done    # ... of a failed build too: no compiler is left writing into $OUT
[ "$failed" -eq 0 ] || exit "$failed"        # a failed translation unit fails the build, before any link
link libtactile_gym_hip.so "${PRODUCT_OBJS[@]}"
link libtactile_gym_hip_test.so "${TEST_OBJS[@]}"
[ "$DRY" = "1" ] || echo "built $OUT/libtactile_gym_hip.so $OUT/libtactile_gym_hip_test.so"
