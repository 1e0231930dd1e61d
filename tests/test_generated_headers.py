"""The generated inline-asm headers are what their generators write: tools/gen_field_asm.py and tools/gen_keccak_asm.py, run into a
temporary file, reproduce myzkp_amd/csrc/mzk_field_asm.h and mzk_keccak_asm.h byte for byte.  A fix to an asm block made in the
header instead of the generator would be lost at the next regeneration (myzkp_amd/build.py regenerates a header whenever its
generator is newer); this keeps the two together.  CPU only."""
import os, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("gen,header", [("gen_field_asm.py", "mzk_field_asm.h"), ("gen_keccak_asm.py", "mzk_keccak_asm.h")])
def test_generator_reproduces_the_committed_header(tmp_path, gen, header):
    out = tmp_path / header
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", gen), str(out)], check=True, capture_output=True, cwd=str(tmp_path))
    want = open(os.path.join(ROOT, "myzkp_amd", "csrc", header), "rb").read()
    got = out.read_bytes()
    assert got == want, "%s is not what tools/%s writes: change the generator and regenerate the header" % (header, gen)
