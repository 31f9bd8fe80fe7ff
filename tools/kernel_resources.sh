#!/bin/sh
# Registers (vector and scalar), private segment, LDS and occupancy of every kernel of a HIP source file, from the compiler's
# -Rpass-analysis=kernel-resource-usage remarks (device-only compile for gfx950: needs no GPU, writes no object).
#   tools/kernel_resources.sh [file.hip] [kernel-name-pattern]
# default: the edge passes, cuda-bundle-adjustment_amd/csrc/kernels/ba_kernels.hip, every kernel.
# A private segment ("scratch") other than 0 on a kernel of the fused iteration is a finding: DESIGN.md section 4.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
SRC=${1:-$ROOT/cuda-bundle-adjustment_amd/csrc/kernels/ba_kernels.hip}
PAT=${2:-.}
HIPCC=${HIPCC:-hipcc}
ARCH=${ARCH:-gfx950}
# the product's flags (cuda-bundle-adjustment_amd/Makefile); the Cholesky and covariance kernels contract
FLAGS="-O3 -std=c++17 -fPIC -Wno-unused-function -Wno-pass-failed -ffp-contract=off"
case "$SRC" in *chol_kernels.hip | *cov_kernels.hip) FLAGS="$FLAGS -ffp-contract=fast" ;; esac
"$HIPCC" --offload-arch="$ARCH" $FLAGS --offload-device-only -Rpass-analysis=kernel-resource-usage -c "$SRC" -o /dev/null 2>&1 |
    awk -v pat="$PAT" '
    function flush() {
        if (name != "" && name ~ pat)
            printf "%-6s %-6s %-8s %-8s %-6s %s\n", vgpr, sgpr, scratch, lds, occ, name
        name = ""
    }
    BEGIN { printf "%-6s %-6s %-8s %-8s %-6s %s\n", "VGPRs", "SGPRs", "scratch", "LDS", "waves", "kernel  (scratch, LDS: bytes per lane / per workgroup; waves per SIMD)" }
    /remark:.*Function Name:/ { flush(); name = $0; sub(/.*Function Name: */, "", name); sub(/ *\[-Rpass.*/, "", name) }
    /remark:.* VGPRs:/ && !/AGPRs/ { v = $0; sub(/.* VGPRs: */, "", v); sub(/ .*/, "", v); vgpr = v }
    /remark:.*TotalSGPRs:/ { v = $0; sub(/.*TotalSGPRs: */, "", v); sub(/ .*/, "", v); sgpr = v }
    /remark:.*ScratchSize \[bytes\/lane\]:/ { v = $0; sub(/.*: */, "", v); sub(/ .*/, "", v); scratch = v }
    /remark:.*LDS Size \[bytes\/block\]:/ { v = $0; sub(/.*: */, "", v); sub(/ .*/, "", v); lds = v }
    /remark:.*Occupancy \[waves\/SIMD\]:/ { v = $0; sub(/.*: */, "", v); sub(/ .*/, "", v); occ = v }
    END { flush() }' | { if command -v c++filt > /dev/null; then c++filt; else cat; fi; }
