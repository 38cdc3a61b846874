"""What the host tests of the fused passes ask hipcc about one translation unit: the kernels it emits, what each needs, and the
gfx950 assembly.  Needs no GPU (hipcc cross-compiles)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "compute-engine_amd", "csrc")
RESOURCE_KEYS = ("ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "VGPRs Spill", "SGPRs Spill")


def scalar_memory_write(word: str) -> bool:
    """An SMEM mnemonic that writes or invalidates memory (the store / atomic forms and the data-cache write-back / discard)."""
    w = word.lower()
    return w.startswith("s_") and ("store" in w or "atomic" in w or w.startswith("s_dcache"))


def sources_with_scalar_memory_writes(files):
    """Those of `files` (names under csrc/) whose text holds such a mnemonic anywhere, a comment or a string included."""
    def words(f):
        return re.findall(r"\b[sS]_[A-Za-z0-9_]+", open(os.path.join(CSRC, f)).read())
    return [f for f in files if any(scalar_memory_write(w) for w in words(f))]


def compile_unit(source):
    """Compiles csrc/`source` as the product build does, device code only.  Returns (kernels, resources, text, mnemonics): the
    kernel names in the order hipcc reports them, {key of RESOURCE_KEYS: one value per kernel, as strings}, the assembly text,
    and the set of instruction mnemonics in it.  Skips the calling test where there is no hipcc."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc is not here")
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "unit.s")
        r = subprocess.run([hipcc, "-DLCE_PRODUCT_BUILD", "-O3", "-std=c++17", "-ffp-contract=off", "--offload-arch=gfx950",
                            "-I", CSRC, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", "-o", asm,
                            os.path.join(CSRC, source)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(asm).read()
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    resources = {key: re.findall(re.escape(key) + r": (\d+)", r.stderr) for key in RESOURCE_KEYS}
    return kernels, resources, text, set(re.findall(r"^\s+([a-z]+_[a-z0-9_]+)", text, re.M))
