#!/usr/bin/env bash
# Build an EXPERIMENT variant of the library next to the product one: same sources, extra -D flags, own object dir and name.
#   tools/build_experiment.sh <name> <flags...>      ->  adaptigraph_amd/csrc/libadaptigraph_hip_<name>.so
# Loaded with ADAPTIGRAPH_AMD_LIB=<path> by tools/ only; never by the product package or the tests.
# The source list and the flags have one home: adaptigraph_amd/csrc/build.sh.
set -euo pipefail
exec bash "$(dirname "$0")/../adaptigraph_amd/csrc/build.sh" experiment "$@"
