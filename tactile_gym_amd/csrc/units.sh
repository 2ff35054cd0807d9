# Sourced by build.sh and relink.sh, from this directory: what both take from the environment, the table of translation units (units.txt), and
# the one place where a compiler command is run - or, under TG_DRY_RUN=1, printed.
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
OUT=${TG_OUT:-../lib}
UNITS=(); UNIT_FLAGS=(); PRODUCT_OBJS=(); TEST_OBJS=(); both=()      # UNIT_FLAGS[i]: the extra flags of UNITS[i]
while read -r name library flags; do
    case $name in ''|'#'*) continue ;; esac
    flags=${flags%%#*}
    case $library in
        product) PRODUCT_OBJS+=("$OUT/$name.o") ;;
        test)    TEST_OBJS+=("$OUT/$name.o") ;;
        both)    PRODUCT_OBJS+=("$OUT/$name.o"); both+=("$OUT/$name.o") ;;
        *)       echo "units.txt: $name: library '$library' is not product, test or both" >&2; exit 2 ;;
    esac
    UNITS+=("$name"); UNIT_FLAGS+=("$flags")
done < units.txt
TEST_OBJS+=("${both[@]}")
DRY=${TG_DRY_RUN:-0}
run() { if [ "$DRY" = "1" ]; then echo "$*"; else "$@"; fi; }
link() {    # link <library file> <objects...>
    local lib=$1; shift
    run $HIPCC --offload-arch=gfx950 -shared -fPIC "$@" -o "$OUT/$lib"
}
