"""The host side of csrc/mcq_api.hip without a GPU and without an interpreter process: tests/layout_check.cpp compiles the translation unit into a
stand-alone program under AddressSanitizer and UBSan and holds the scratch layouts (the Arena and the *_layout functions) to the formulas the
entries carried before, and the structural scan of mcq_les_scalings / mcq_les_scalings_open to its return codes and messages on 1 and 3 threads.
The kernels the translation unit names are taken from the SIMT interpreter's library; none is launched."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scratch_layouts_and_structural_scan(emu_lib, tmp_path):
    exe = str(tmp_path / "layout_check")
    emu = os.path.dirname(emu_lib)
    subprocess.run(["g++", "-O0", "-g", "-std=c++17", "-pthread", "-x", "c++", "-Wno-unused-result", "-Wno-attributes", "-Wno-psabi",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-I", os.path.join(emu, "include"),
                    os.path.join(ROOT, "tests", "layout_check.cpp"), "-o", exe, "-L", emu, "-l:" + os.path.basename(emu_lib), "-Wl,-rpath," + emu, "-ldl"],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True)       # (the sanitizers' runtimes are linked into the program itself)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
