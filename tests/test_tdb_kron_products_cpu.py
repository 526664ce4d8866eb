"""CPU: the structured time-dependent path's product modes (k_tdb_kron_product, csrc/dto_tdb_kron.hip) as far
as they show without a device -- the words (the header's option paragraph, the DESIGN section and Evaluator.set_option's doc name
the structured path as served, the sentence that excluded it is gone), and the compiler's resource remarks for the kernel file
(every kernel without vector spill or scratch within 256 VGPRs, four product instantiations beside the four value ones).  The
remarks alone are read, not the assembly.  hipcc cross-compiles without a GPU."""
import os
import re
import subprocess

import pytest

import dto_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc", "dto_tdb_kron.hip")
H = open(os.path.join(ROOT, "include", "dto_engine.h"), encoding="utf-8").read()
DESIGN = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
OPTION = "tdb_matrix_free_products"


def _option_paragraph():
    start = H.index('"%s" (default 0)' % OPTION)
    return re.sub(r"\s*\n \*\s+", " ", H[start:H.index('"debug_bad_launch"', start)])


def test_the_header_names_the_structured_path_as_served():
    par = _option_paragraph()
    assert "DTO_FLAG_BLOCK_GENERATORS" in par and "structured" in par
    assert "goes matrix-free as a whole" in par
    assert "External integrators and constraints keep the slab route" in par


def test_the_sentence_that_excluded_the_structured_path_is_gone():
    flat = re.sub(r"\s*\n \*\s+", " ", H)
    assert "integrators on the structured time-dependent path, keep the slab route" not in flat
    assert "without DTO_FLAG_BLOCK_GENERATORS structure" not in flat
    src = open(os.path.join(ROOT, "directtrajopt.jl_amd", "csrc", "dto_engine.cpp"), encoding="utf-8").read()
    assert "has no product modes" not in src and "!t.kron;" not in src


def test_the_profile_and_grid_paragraphs_cover_the_product_kernel():
    flat = re.sub(r"\s*\n \*\s+", " ", H)
    assert re.search(r'"tdb_product" \(.*?dense or structured.*?do not count under "tdb_mfma" or "tdb_kron"\)', flat)
    assert re.search(r'"tdb_resident" \(default 0.*?k_tdb_kron_product', flat)


def test_set_option_doc_names_the_structured_path():
    doc = " ".join(dto_amd.Evaluator.set_option.__doc__.split())
    assert OPTION in doc and "structured path" in doc and "block_generators" in doc


def test_design_has_the_section():
    m = re.search(r"^### 4\.24 [^\n]*structured time-dependent path[^\n]*\n(.*?)(?=^##)", DESIGN, flags=re.S | re.M)
    assert m, "DESIGN 4.24 is missing"
    sec = m.group(1)
    for word in ("k_tdb_kron_product", "need = 3", "need = 4", "tdbk_product_layout", "launch_tdb_jtv_place", "VGPR", OPTION):
        assert word in sec, word
    # the value kernel's figures, before and after
    for row in ("| `k_tdb_kron<1>` | 161 | 0 | 0 | 2368 | 2 |", "| `k_tdb_kron<4>` | 256 | 0 | 0 | 41280 | 1 |"):
        assert row[:-1] in sec, row   # (the row goes on with the figures after the change)
    assert len(re.findall(r"^\| `k_tdb_kron_product<[1-4]>` \|", sec, flags=re.M)) == 4
    old = DESIGN[DESIGN.index("### 4.21 "):DESIGN.index("### 4.22 ")]
    assert "have no product modes" not in " ".join(old.split())


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = tmp_path_factory.mktemp("tdbk") / "tdb_kron.o"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-I", os.path.dirname(SRC), SRC, "-o", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            kernels[name][m.group(1).strip()] = int(m.group(2))
    return kernels


def _instances(kernels, stem):
    out = {}
    for nm, figures in kernels.items():
        m = re.match(r"_ZN3dto12_GLOBAL__N_1\d+%sILi(\d)EEEv" % stem, nm)
        if m:
            out[int(m.group(1))] = figures
    return out


def test_every_kernel_is_free_of_vector_spill_and_scratch(remarks):
    assert len(remarks) == 8, sorted(remarks)
    for nm, f in remarks.items():
        assert f["VGPRs Spill"] == 0 and f["ScratchSize"] == 0 and f["VGPRs"] <= 256, (nm, f)


def test_four_product_instantiations_beside_the_value_kernel_s_figures(remarks):
    prod = _instances(remarks, "k_tdb_kron_product")
    assert sorted(prod) == [1, 2, 3, 4], sorted(remarks)
    val = _instances(remarks, "k_tdb_kron")
    # the value kernel's register allocation is what it was before the product kernel joined the file
    got = {mt: (f["VGPRs"], f["VGPRs Spill"], f["ScratchSize"], f["LDS Size"], f["Occupancy"]) for mt, f in val.items()}
    assert got == {1: (161, 0, 0, 2368, 2), 2: (189, 0, 0, 12608, 2), 3: (234, 0, 0, 18752, 1), 4: (256, 0, 0, 41280, 1)}, got
