"""Static counts of kernel variant 11's text (nerfh_mlp_sel.hip), through tools/mfma_free_valu.py and tools/mfma_read_distance.py.

No GPU: the unit is cross-compiled for gfx950 to assembly, once for this file.  The bounds are those the variant was specified with:
the counts of a build in which the 16-way select chains of the PrecX3M16 head extraction are gone (3 759 vector instructions in the
fine kernel, 125 v_cndmask + v_cmp) plus about 1 %; variant 10's fine kernel has 4 023 and 294.  A build that misses them has not
removed the chains.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import mfma_free_valu  # noqa: E402
import mfma_read_distance  # noqa: E402

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
CSRC = os.path.join(ROOT, "dfnet_amd", "csrc")


def _compile(tmp, name, *flags):
    """nerfh_mlp_sel.hip -> (assembly path, the compiler's resource remarks)"""
    out = os.path.join(tmp, name + ".s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", *flags, os.path.join(CSRC, "nerfh_mlp_sel.hip"), "-o", out],
                       cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    return out, p.stderr


def _resources(remarks):
    """{kernel name: {remark: value}} of -Rpass-analysis=kernel-resource-usage"""
    res, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return res


def _kernels(path, remarks):
    rec = {}
    for r in mfma_free_valu.report(path):
        kind = "fine" if "nerfh_fine_sel_kernel" in r["kernel"] else "coarse" if "nerfh_coarse_sel_kernel" in r["kernel"] else None
        if kind:
            rec[kind] = r
    for name, body in mfma_free_valu.kernels(open(path).read().splitlines()):
        kind = "fine" if "nerfh_fine_sel_kernel" in name else "coarse" if "nerfh_coarse_sel_kernel" in name else None
        if kind:
            rec[kind]["read_distance"] = min(mfma_read_distance.scan(body)[1])
            rec[kind]["resources"] = next(v for k, v in _resources(remarks).items() if k == name)
    assert set(rec) == {"fine", "coarse"}, sorted(rec)
    return rec


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the two kernels of the unit as shipped"""
    rec = _kernels(*_compile(str(tmp_path_factory.mktemp("seam")), "sel"))
    for kind in ("fine", "coarse"):
        print(kind, {k: v for k, v in rec[kind].items() if k != "stretches40"})
    return rec


def test_the_select_chains_are_gone(built):
    f = built["fine"]
    assert f["valu"] <= 3800, f["valu"]
    assert f["writelane"] == 0
    assert f["cndmask"] + f["cmp"] <= 140, (f["cndmask"], f["cmp"])


@pytest.mark.parametrize("kind,mfma", (("fine", 1920), ("coarse", 1560)))
def test_resources_and_mfma_counts(built, kind, mfma):
    k = built[kind]
    r = k["resources"]
    assert k["mfma"] == mfma
    assert r["VGPRs"] <= 256 and r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, r
    assert r["Occupancy [waves/SIMD]"] == 2, r
    assert k["read_distance"] >= 6, k["read_distance"]
