#!/bin/bash
# tools/build_variant.sh NAME [extra hipcc flags...] (always -DRVC_EXPERIMENTS: env knobs read, rvc_debug_* exported) : builds comfy-rvc_amd/csrc/variants/librvc_hip_NAME.so for A/B kernel timing
# (the source list and the per-file flags are csrc/Makefile's)
set -e
name=$1; shift
make -C "$(dirname "$0")/../comfy-rvc_amd/csrc" -j16 VARIANT="$name" EXTRA="$*"
echo built variants/librvc_hip_$name.so
