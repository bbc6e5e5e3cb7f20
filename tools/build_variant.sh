#!/bin/bash
# Build an experimental variant of libfheregex.so with extra flags for every .hip:
#   tools/build_variant.sh NAME [-DFOO=1 ...]  ->  fhe-regex_amd/build/exp/lib_NAME.so
# (select it at run time with FHEREGEX_LIB=...; PAIR_SCHED=... in the environment overrides the pair TU's scheduler)
set -e
cd "$(dirname "$0")/../fhe-regex_amd"
name=$1; shift
make -s -j8 BUILD="build/exp/$name" LIB="build/exp/lib_$name.so" HIPFLAGS_EXTRA="$*" >/dev/null
echo "built fhe-regex_amd/build/exp/lib_$name.so"
