#!/bin/bash
# Build a VARIANT of libvvhip.so into videovanish_amd/csrc/ab/<name>.so (git-ignored) without touching the product build, for an interleaved A/B of two
# libraries (tools/ab_libs.sh, tools/bench_with_lib.py, tools/pytest_with_lib.py):
#   tools/build_variant.sh <name> [--src DIR] [extra hipcc flags]
# --src DIR: the videovanish_amd/csrc of a tree at another revision (`git archive REV videovanish_amd/csrc include | tar -x -C /tmp/rev`, then
# --src /tmp/rev/videovanish_amd/csrc); default: this tree's own.  The sources and their flags are listed in one place, videovanish_amd/csrc/build.sh.
set -e
NAME=$1; shift
CSRC=$(cd "$(dirname "$0")/.." && pwd)/videovanish_amd/csrc
bash $CSRC/build.sh --out $CSRC/ab/$NAME.so "$@"
