#!/bin/bash
# Builds libkc_hip.so with extra device-compile flags into
# kmer-counter_amd/variants/<name>/ (tuning experiments; select with KC_LIB).
# Variants are experiment builds (-DKC_EXPERIMENTS, device and host code): they
# honour the timing ablation variables (KC_F_SKIP, KC_P2_SKIP, KC_P5_SKIP,
# KC_SEG_SKIP, KC_SKM_MMIN) that the release library ignores.
# usage: tools/build_variant.sh <name> "<hipcc flags>"
set -e
[ -n "$1" ] || { echo "usage: $0 <name> \"<hipcc flags>\"" >&2; exit 2; }
R=$(cd "$(dirname "$0")/../kmer-counter_amd" && pwd)
D=${VARIANT_DIR:-$R/variants}/$1
mkdir -p "$D" && D=$(cd "$D" && pwd)
make -C "$R" -s -j8 ARCH=gfx950 OUT="$D/" EXTRA_DEFS=-DKC_EXPERIMENTS EXTRA_HIPFLAGS="$2" lib
rm -rf "$D/build"
echo built $D/libkc_hip.so
