#!/bin/bash
# build_variant.sh NAME "EXTRA FLAGS" [WAVES=4] -- tuning / profiling build of the HIP library under samsim_amd/csrc/variants/
# (selected at run time with SAMSIM_HIP_LIB=...; never the product library).  Sources, flags and the WAVES default are the
# Makefile's: this only calls its `variant` target.
set -e
make -C "$(dirname "$0")/../samsim_amd/csrc" variant NAME="$1" EXTRA="$2" ${3:+WAVES="$3"}
