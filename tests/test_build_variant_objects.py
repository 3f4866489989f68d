"""tools/build_variant.sh links the A/B variants (libact_<name>.so, loaded through ACT_LIB_PATH by ab_bench.sh, pmc_ab.sh,
profile_round.sh) by hand: every host object the product library links (csrc/Makefile OBJS beyond the HIP sources) must be made
and linked there too, or capi.load() of a variant fails on the entry points that object provides."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_variants_link_every_host_object_of_the_product():
    mk = open(os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc", "Makefile")).read()
    objs = re.search(r"^OBJS := \$\(SRCS:\.hip=\.o\) (.*)$", mk, re.M).group(1).split()
    assert "node.o" in objs and "node_nullifier.o" in objs, objs
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    make_line = re.search(r'^make -C "\$src" (.*?) >/dev/null$', sh, re.M).group(1).split()
    link_line = next(l for l in sh.splitlines() if l.startswith("hipcc --offload-arch=gfx950 -shared"))
    for o in objs:
        assert o in make_line, (o, "not made by build_variant.sh")
        assert f'"$src/{o}"' in link_line, (o, "not linked by build_variant.sh")


def test_variants_compile_every_hip_unit_of_the_product():
    """... and every HIP unit of the Makefile's SRCS must be compiled by the script's loop (its objects are linked as build/<name>/*.o):
    a variant without k_admit, k_copies, k_replay, ... lacks their launchers and does not load.  The units built with the range
    kernel's flags in the product (Makefile: TUFLAGS := $(BITSFLAGS)) must take the script's BITS flags as well."""
    mk = open(os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert len(srcs) >= 16 and all(s.endswith(".hip") for s in srcs), srcs
    for s in srcs:
        assert os.path.exists(os.path.join(ROOT, "anonymous-credit-tokens_amd", "csrc", s)), s
    sh = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    units = re.search(r"^for f in (.*?); do$", sh, re.M).group(1).split()
    assert sorted(units) == sorted(s[:-4] for s in srcs), set(units) ^ set(s[:-4] for s in srcs)
    assert '-c "$src/$f.hip" -o "$out/$f.o"' in sh and '"$out"/*.o' in sh
    bits_units = sorted(o[:-2] for l in re.findall(r"^(.*): TUFLAGS := \$\(BITSFLAGS\)$", mk, re.M) for o in l.split() if not o.startswith("fast_"))
    assert "k_spend_bits" in bits_units
    bits_line = next(l for l in sh.splitlines() if "${BITS--DACT_FE_PAIR_ASM}" in l)
    assert sorted(re.findall(r'"\$f" = (\w+)', bits_line)) == bits_units, (bits_line, bits_units)
