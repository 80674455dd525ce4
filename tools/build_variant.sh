#!/bin/bash
# Build an A/B variant of the library in-tree:  tools/build_variant.sh NAME [extra hipcc flags]  ->  graspnerf_amd/csrc/libgnr_NAME.so
# (selected at load time with GNR_LIB=libgnr_NAME.so; tools/ab_chain.py times a list of them in one GPU call).  The same sources and
# flags as the product (graspnerf_amd/csrc/sources.sh), so a variant resolves every symbol the Python front end binds.
set -e
NAME=$1; shift
cd "$(dirname "$0")/../graspnerf_amd/csrc"
. ./sources.sh
hipcc $FLAGS -o libgnr_$NAME.so $SRC "$@"
