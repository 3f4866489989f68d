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
