#!/usr/bin/env bash
# tests/native/host_side_check.cpp (the host pool and the compact-plan expansion, no GPU involved) under the
# sanitizers: one build with ASan + UBSan, one with TSan, each a stand-alone executable run under a time limit.
# Run by hand on a CPU machine; no test calls it.  usage: tools/host_side_sanitize.sh   (CXX=clang++ to override)
set -euo pipefail
REPO="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
CXX="${CXX:-g++}"
SRC="${REPO}/tests/native/host_side_check.cpp"
OUT="$(mktemp -d)"
trap 'rm -rf "${OUT}"' EXIT
"${CXX}" -std=c++17 -pthread -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o "${OUT}/check_asan_ubsan" "${SRC}" &&
  echo "== ASan + UBSan" && timeout -k 10 300 "${OUT}/check_asan_ubsan" &&
  "${CXX}" -std=c++17 -pthread -O1 -g -fsanitize=thread -o "${OUT}/check_tsan" "${SRC}" &&
  echo "== TSan" && timeout -k 10 300 "${OUT}/check_tsan" &&
  echo "host_side_sanitize: both builds ran clean"
