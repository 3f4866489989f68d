#!/bin/bash
# tools/build_variant.sh <name> [extra hipcc flags...] -- builds anonymous-credit-tokens_amd/libact_<name>.so (same sources, extra -D flags)
# for same-box A/B runs (tools/ab_bench.sh <name>...).  Objects go to build/<name>/ (git-ignored).
set -e
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
src=$root/anonymous-credit-tokens_amd/csrc
out=$root/build/$name
mkdir -p "$out"
make -C "$src" host_hash.o host_pool.o node.o node_nullifier.o node_issue_wire.o node_keyring.o node_epochs.o >/dev/null
pids=()
# FILES="k_spend_verify ..." restricts the extra flags to those translation units (default: all)
for f in engine k_misc k_spend_verify k_spend_bits k_sign k_prove k_client k_client_ring k_keyring k_admit k_copies k_cbor_read k_replay k_admit_replay k_return_replay k_reserve k_debug_fe k_debug_fe_pair k_debug_sc k_debug_secret; do
  extra=("$@")
  if [ -n "$FILES" ] && ! [[ " $FILES " == *" $f "* ]]; then extra=(); fi
  # the range kernel's unit is built pair-interleaved in the product (csrc/Makefile BITSFLAGS); BITS= overrides that for A/B ("BITS=" = per-column form)
  # (k_debug_fe_pair is the field-form test kernel in the range kernel's form: tests/test_gpu_fe_forms.py then tests what a variant runs)
  if [ "$f" = k_spend_bits ] || [ "$f" = k_debug_fe_pair ]; then extra+=(${BITS--DACT_FE_PAIR_ASM}); fi
  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wno-unused-function -Wno-pass-failed -Wno-unused-value -DACT_CT_SECRET_TABLES "${extra[@]}" -c "$src/$f.hip" -o "$out/$f.o" &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
extra_libs=()
[[ " $* " == *" -DACT_ROCTX "* ]] && extra_libs=(-L/opt/rocm/lib -lrocprofiler-sdk-roctx)      # named ranges for rocprofv3 --marker-trace
hipcc --offload-arch=gfx950 -shared -fPIC -o "$root/anonymous-credit-tokens_amd/libact_$name.so" "$out"/*.o "$src/host_hash.o" "$src/host_pool.o" "$src/node.o" "$src/node_nullifier.o" "$src/node_issue_wire.o" "$src/node_keyring.o" "$src/node_epochs.o" -lpthread "${extra_libs[@]}"
echo "built libact_$name.so"
