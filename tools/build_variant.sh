#!/bin/bash
# Builds an A/B variant of libgsv.so with extra -D flags (sources in $VSRCS, default ecrecover notary)
# into variants/<name>/ (git-ignored,
# shipped to the GPU box); select it at run time with GSV_LIB_PATH=variants/<name>/libgsv.so.
# The unit list, the compiler and the flags are the Makefile's (make -s print-SRCS ...).
set -e
name=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p $R/variants/$name
cd $R/geth-sharding_amd/csrc
make -s -j8 >/dev/null
HIPCC=$(make -s print-HIPCC); BASE=$(make -s print-BASE); LIBS=$(make -s print-LIBS)
VSRCS=${VSRCS:-ecrecover notary}
for f in $VSRCS; do
    $HIPCC "$@" $BASE -c $f.hip -o $R/variants/$name/$f.o 2>&1 | grep -v hip-link || true &
done
wait
objs=""
for f in $(make -s print-SRCS | sed 's/\.hip//g'); do
    case " $VSRCS " in *" $f "*) ;; *) cp build/$f.o $R/variants/$name/ ;; esac
    objs="$objs $R/variants/$name/$f.o"
done
$HIPCC $BASE -shared -o $R/variants/$name/libgsv.so $objs $LIBS
echo built $R/variants/$name/libgsv.so
