#!/bin/bash
# Developer A/B builds of libaa_interp.so: tools/ab_build.sh NAME "-DFLAG=1 ..." [object.o ...]
# Recompiles the listed objects (default: the headline u8 kernel's, aa_fused_u8_v3_c3.o) with the extra flags into build_ab/NAME/,
# using the Makefile's own compile command for each, and links them with the stock objects (every object the Makefile links, so run
# make first) into interpolate_antialiasing_amd/csrc/libaa_interp_NAME.so.
# Use with AA_INTERP_LIB=.../libaa_interp_NAME.so (see _lib.py).  Not part of the product build.
set -e
NAME=$1; FLAGS=$2; shift 2 || true
PICK=${@:-aa_fused_u8_v3_c3.o}
cd "$(dirname "$0")/../interpolate_antialiasing_amd/csrc"
mkdir -p build_ab/$NAME
OBJS=""
for o in $(make -s print-objs); do
  if echo " $PICK " | grep -q " $o "; then
    CMD=$(make -s -n -B TUNING="$FLAGS" "$o" | grep hipcc)
    eval "${CMD% -o *} -o build_ab/$NAME/$o" &
    OBJS="$OBJS build_ab/$NAME/$o"
  else
    OBJS="$OBJS $o"
  fi
done
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o libaa_interp_$NAME.so $OBJS
echo built libaa_interp_$NAME.so
