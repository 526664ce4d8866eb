"""CPU: what only the ISA shows about the replicated-block kernel (csrc/dto_kron.hip): its products run on the FP64 matrix
instruction, every instance, and nothing between the first and the last of them goes through scratch memory (the fragments
and accumulators of a wave tile live in registers).  hipcc cross-compiles without a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc", "dto_kron.hip")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "kron.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-I", os.path.dirname(SRC), SRC, "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return out.read_text()


def test_products_are_mfma_and_stay_out_of_scratch(isa):
    names = re.findall(r"^(_ZN3dto12_GLOBAL__N_16k_kronILi(\d)EEEvNS0_8KronArgsE):", isa, re.M)
    assert sorted(int(mt) for _, mt in names) == [1, 2, 3, 4], names
    for nm, mt in names:
        mt = int(mt)
        body = isa[isa.index(nm + ":"):]
        body = body[:body.index(".Lfunc_end")].split("\n")
        mf = [k for k, l in enumerate(body) if "v_mfma_f64_16x16x4_f64" in l]
        # a wave tile is MT accumulators x 4 MT k-steps; several product sites (sweep, extras, products outside the sweep)
        assert len(mf) >= 4 * mt * mt and len(mf) % (4 * mt * mt) == 0, (nm, len(mf))
        inside = body[mf[0]:mf[-1] + 1]
        assert not any("scratch_" in l for l in inside), nm
        meta = isa[isa.index(".amdhsa_kernel " + nm):]
        assert int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", meta).group(1)) <= 256, nm   # a workgroup is one wave per SIMD: two workgroups per CU
