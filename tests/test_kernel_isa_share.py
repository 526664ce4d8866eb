"""CPU: what only the ISA shows about the replication kernel of DTO_FLAG_SHARED_GENERATORS (csrc/dto_share.hip): the copy moves
16 bytes per lane in both directions, every memory write is a vector store, and nothing is accumulated (one writer per entry: no
atomic of any kind).  hipcc cross-compiles without a GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "directtrajopt.jl_amd", "csrc", "dto_share.hip")


@pytest.fixture(scope="module")
def body(tmp_path_factory):
    out = tmp_path_factory.mktemp("isa") / "share.s"
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-I", os.path.dirname(SRC), SRC, "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    isa = out.read_text()
    names = re.findall(r"^(\w*k_share_E\w*):", isa, re.M)
    assert len(names) == 1, names
    b = isa[isa.index(names[0] + ":"):]
    return [l.split(";")[0].strip() for l in b[:b.index(".Lfunc_end")].split("\n")]


def test_the_copy_moves_sixteen_bytes_per_lane(body):
    assert any(l.startswith("global_load_dwordx4") for l in body)
    assert any(l.startswith("global_store_dwordx4") for l in body)
    # the odd head and tail entries are 8 bytes wide; no store is narrower
    assert not any(re.match(r"(global|flat|buffer)_store_(dword|short|byte)\b", l) for l in body)


def test_every_memory_write_is_a_plain_vector_store(body):
    assert not any(re.match(r"s_\w*(store|atomic|dcache)", l) for l in body), "a scalar-unit memory write"
    assert not any("atomic" in l for l in body), "an atomic"
    assert not any(l.startswith("scratch_") for l in body), "spills"
    stores = [l for l in body if re.match(r"\w+_store_", l)]
    assert stores and all(l.startswith("global_store_dwordx") for l in stores), stores
