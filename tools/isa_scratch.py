"""Per-kernel register / scratch census of one HIP source compiled for gfx950 (device ISA only):
    python tools/isa_scratch.py multimodal-sam-adapter_amd/csrc/gemm_v2.hip [-DX ...]
prints, per kernel: scratch_ instructions, VGPRs, scratch bytes, s_waitcnt vmcnt(0) count, v_readlane count and a digest of its instruction stream (sha1 over
the instruction lines: comments, directives / local labels, blank lines and the per-invocation __hip_cuid_ symbol left out -- equal digests = the same kernel; with
--digest only "digest vgprs scratch_bytes kernel", the form of profiles/gemm_shared_header_isa.txt).  Used by
tests/test_host_cpu.py::test_gemm_kernels_do_not_spill (a scratch reload in front of an LDS-DMA drains the prefetch stream)."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-fno-slp-vectorize", "-w", "-S", "--cuda-device-only"]


def demangle_template(name):
    """_Z14gemm_v2_kernelILb0ELi1ELb1ELi8ELi3EEv10GemmV2Args -> gemm_v2_kernel<0,1,1,8,3> (enough for the kernels of this library)"""
    m = re.match(r"_Z\d+([A-Za-z_0-9]+?)I(.*)Ev", name)
    if not m:
        return name
    args = re.findall(r"L[bi](n?\d+)E", m.group(2))
    return m.group(1) + "<" + ",".join(a.replace("n", "-") for a in args) + ">"


def census(src, extra=()):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + list(extra) + ["-o", out, src], check=True, stderr=subprocess.DEVNULL)
        res, name = {}, None
        for line in open(out):
            m = re.match(r"^(_Z\S+):", line)
            if m:
                name = demangle_template(m.group(1))
                res[name] = dict(scratch=0, vgprs=0, scratch_bytes=0, vmcnt0=0, readlane=0, lines=0, mfma_f16=0, mfma_scale_f8=0, sha=hashlib.sha1())
            if name is None:
                continue
            r = res[name]
            r["lines"] += 1
            if line.strip() and not line.lstrip().startswith((";", ".")) and "__hip_cuid_" not in line:
                r["sha"].update(line.strip().encode() + b"\n")
            if "scratch_" in line and not line.lstrip().startswith((";", ".")):
                r["scratch"] += 1
            if "s_waitcnt vmcnt(0)" in line:
                r["vmcnt0"] += 1
            if "v_readlane_b32" in line:
                r["readlane"] += 1
            if "v_mfma_f32_16x16x32_f16" in line:
                r["mfma_f16"] += 1
            if "v_mfma_scale_f32_16x16x128_f8f6f4" in line:
                r["mfma_scale_f8"] += 1
            m2 = re.search(r"; NumVgprs: (\d+)", line)
            if m2:
                r["vgprs"] = int(m2.group(1))
            m3 = re.search(r"; ScratchSize: (\d+)", line)
            if m3:
                r["scratch_bytes"] = int(m3.group(1))
                r["digest"] = r.pop("sha").hexdigest()
                name = None
        return res


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x != "--digest"]
    for k, v in census(args[0], args[1:]).items():
        if "--digest" in sys.argv:
            print(f"{v['digest']}  vgprs {v['vgprs']:3d}  scratch_bytes {v['scratch_bytes']:4d}  {k}")
            continue
        print(f"{k:44s} scratch_instr {v['scratch']:4d}  vgprs {v['vgprs']:3d}  scratch_bytes {v['scratch_bytes']:4d}  vmcnt(0) {v['vmcnt0']:3d}  readlane {v['readlane']:4d}  lines {v['lines']}  {v['digest'][:12]}")
