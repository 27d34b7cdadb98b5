"""hipcc's per-kernel resource remarks for one file of reagent_amd/csrc (test infrastructure): compile it for gfx950 with
-Rpass-analysis=kernel-resource-usage and parse what the compiler reports for every kernel."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KEYS = ("VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "VGPRs")


def kernel_resources(hip_file, tmp_path):
    """-> {mangled kernel name: {key of KEYS: value}} for reagent_amd/csrc/<hip_file>"""
    csrc = os.path.join(ROOT, "reagent_amd", "csrc")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{csrc}", f"-I{ROOT}/include",
                          "-Wno-unused-result", "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, hip_file),
                          "-o", str(tmp_path / "o.o")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    kernels, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            kernels[name] = {}
        for key in KEYS:
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name:
                kernels[name].setdefault(key, int(m.group(1)))
    return kernels

