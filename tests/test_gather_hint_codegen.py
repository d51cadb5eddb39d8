"""The hinted gather of gnx_spmm_device.h must reach the assembler as BOTH a plain and a non-temporal global_load_dwordx4: a
source-level choice between the two does not (the compiler merges them into one plain load, or speculates both), which is why the
statement is inline asm.  Compiles a small unit for gfx950 and reads its assembly; no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)

UNIT = r"""
#include "gnx_spmm_device.h"
__global__ void k_unit(const float *X, const int *cols, float *out) {
    f32x4 x[4];
    for (int u = 0; u < 4; ++u) {               // per lane: hot and cold rows share a wave
        const int j = cols[threadIdx.x * 4 + u];
        x[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        gather16_hinted(x[u], X + (int64_t)hint_col(j) * 128, j);
    }
    gather_wait<4>(x);
    f32x4 y[4] = {x[0] + x[1], x[2] + x[3], x[0], x[1]};
    const int ju = __builtin_amdgcn_readfirstlane(cols[0]);   // wave-uniform column: a scalar branch
    gather16_hinted_uniform(y[3], X + (int64_t)hint_col(ju) * 128 + threadIdx.x * 4, ju);
    gather_wait<4>(y);
    *reinterpret_cast<f32x4 *>(out + threadIdx.x * 4) = y[0] + y[1] + y[2] + y[3];
}
"""


@pytest.mark.skipif(HIPCC is None, reason="no hipcc on this machine")
def test_hinted_gather_emits_a_plain_and_a_non_temporal_load(tmp_path):
    src, asm = tmp_path / "unit.hip", tmp_path / "unit.s"
    src.write_text(UNIT)
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I",
                    os.path.join(ROOT, "gnn-tf_amd", "csrc"), str(src), "-o", str(asm)], check=True, capture_output=True)
    body = re.search(r"^_Z6k_unit\w*:.*?s_endpgm", asm.read_text(), re.S | re.M).group(0)
    loads = re.findall(r"^\s*(\w+_load_dwordx4)\s+v\[\d+:\d+\], v\[\d+:\d+\], off(.*)$", body, re.M)
    plain = [kind for kind, tail in loads if kind == "global_load_dwordx4" and tail.strip() == ""]
    cold = [kind for kind, tail in loads if kind == "global_load_dwordx4" and tail.strip() == "nt"]
    assert len(plain) == 5 and len(cold) == 5, loads          # four per-lane statements and the uniform one, both forms each
    assert "flat_load" not in body
    # every gather is waited for by hand before its registers are read: the asm waits are there, after the last gather of a batch
    waits = [m.start() for m in re.finditer(r"s_waitcnt vmcnt\(0\)", body)]
    last_gather = max(m.start() for m in re.finditer(r"global_load_dwordx4", body))
    assert len(waits) >= 2 and waits[-1] > last_gather
    assert "scratch_" not in body
