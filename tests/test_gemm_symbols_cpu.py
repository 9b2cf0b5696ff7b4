"""CPU guard: every gemm*_kernel<...> instantiation in the gfx950 code objects of libivr_hip.so is in the coverage table of
tests/test_gemm_gpu.py, so a new instantiation without a per-element test fails here (clang-offload-bundler and llvm-readelf of the
ROCm LLVM)."""
import os
import re
import struct
import subprocess
import tempfile

from ivr_amd import _ffi
from test_gemm_gpu import COVERAGE

LLVM = "/opt/rocm/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
EPI = {"0": "STORE", "1": "RESID", "2": "PATCH", "3": "F32"}
ACT = {"n1": "none", "0": "QUICK", "1": "GELU"}


def canonical(name, args):
    """gemm_kernel / gemm_big_kernel / gemm_skinny_kernel <T, EPI, ACT[, SKIP | MTL]>, gemm_pers_kernel <EPI, ACT>,
    gemm_big8_kernel <EPI, ACT, OUT8, SKIP> -> the key format of COVERAGE."""
    types = [a for a in args if a in ("t", "f")]
    ints = [a[2:-1] for a in args if a.startswith("Li")]
    bools = [a[2] == "1" for a in args if a.startswith("Lb")]
    parts = [{"t": "bf16", "f": "f32"}[t] for t in types] + [EPI[ints[0]], ACT[ints[1]]]
    if name == "gemm_skinny_kernel":
        parts.append(ints[2])
    if name == "gemm_big8_kernel":
        parts += ["OUT8"] * bools[0] + ["SKIP"] * bools[1]
    elif bools:
        parts += ["SKIP"] * bools[0]
    return f"{name}<{','.join(parts)}>"


def gemm_symbols(lib_path):
    """Demangled-to-key names of the gemm*_kernel functions of every gfx950 code object in the library's .hip_fatbin."""
    sec = subprocess.run([f"{LLVM}/llvm-readelf", "-S", "-W", lib_path], capture_output=True, text=True, check=True).stdout
    m = re.search(r"\.hip_fatbin\s+\S+\s+[0-9a-f]+\s+([0-9a-f]+)\s+([0-9a-f]+)", sec)
    assert m, "no .hip_fatbin section"
    with open(lib_path, "rb") as f:
        f.seek(int(m.group(1), 16))
        data = f.read(int(m.group(2), 16))
    keys = set()
    with tempfile.TemporaryDirectory() as td:
        for i, start in enumerate(mm.start() for mm in re.finditer(re.escape(MAGIC), data)):
            # one bundle per translation unit; the header says how long it is, the bundler takes the gfx950 entry out of it
            n = struct.unpack_from("<Q", data, start + 24)[0]
            q, end, targets = start + 32, start, []
            for _ in range(n):
                off, size, idl = struct.unpack_from("<QQQ", data, q)
                targets.append(data[q + 24:q + 24 + idl].decode())
                end = max(end, start + off + size)
                q += 24 + idl
            tgt = [t for t in targets if t.endswith("gfx950")]
            assert tgt, targets
            src, co = os.path.join(td, f"b{i}.bundle"), os.path.join(td, f"b{i}.co")
            with open(src, "wb") as f:
                f.write(data[start:end])
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={src}", f"--output={co}",
                            f"--targets={tgt[0]}"], check=True)
            syms = subprocess.run([f"{LLVM}/llvm-readelf", "--symbols", "-W", co], capture_output=True, text=True, check=True).stdout
            for line in syms.splitlines():
                mm = re.search(r"_ZN12_GLOBAL__N_1\d+(gemm\w*_kernel)I(\w+?)EEv8GemmArgs$", line)
                if mm and " FUNC " in line:
                    keys.add(canonical(mm.group(1), re.findall(r"Li(?:n?\d+)E|Lb[01]E|[tf]", mm.group(2))))
    return keys


def test_every_gemm_instantiation_is_in_the_coverage_table():
    assert os.path.exists(_ffi.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    found = gemm_symbols(_ffi.LIB_PATH)
    assert len(found) >= 50, sorted(found)
    missing = sorted(found - set(COVERAGE))
    assert not missing, f"GEMM instantiations without a per-element test in tests/test_gemm_gpu.py: {missing}"
    stale = sorted(set(COVERAGE) - found)
    assert not stale, f"coverage table lists instantiations the library does not hold: {stale}"
