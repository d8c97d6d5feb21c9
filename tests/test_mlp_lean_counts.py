"""Static counts of kernel variant 12's text (nerfh_mlp_lean.hip), through tools/mfma_free_valu.py and tools/mfma_read_distance.py.

No GPU: the unit is cross-compiled for gfx950 to assembly, once for this file.  The bounds were set before the first GPU run of each
technique from the counts of the unit without it and what the technique as specified takes out.  A build that misses a bound has not
removed what the unit was specified to remove:
  * one select per head value: a build in which the 16-way select chains of the PrecX3M16 head extraction are gone had 125 v_cndmask +
    v_cmp in the fine kernel, the bound is that plus about 1 % of the kernel's vector instructions; with the chains it had 294, and
    39 SGPRs parked in VGPR lanes (v_writelane_b32: none may remain);
  * the lean seam and guard: 3 754 vector instructions in the fine kernel and 2 707 in the coarse one before them; the packed head
    activations and the paired range guard alone give 3 458 in the fine kernel, the paired guard alone 2 579 in the coarse one;
    v_rcp_iflag_f32 is the reciprocal of the 32-bit division by n_samples, and v_pk_max_u16 the range guard's old instruction, 336 /
    256 per tile before.

As shipped: fine 3 414, coarse 2 556; no v_rcp_iflag_f32; v_pk_max_u16 0 / 0 (v_pk_maximum3_f16 168 / 128); VGPRs 250 / 228; MFMAs
1 920 / 1 560; read distance 6 / 6; eight v_permlane32_swap_b32 in the fine kernel; v_cndmask + v_cmp 60 + 31 / 36 + 24; no v_writelane_b32.
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
KINDS = {"fine": "nerfh_fine_lean_kernel", "coarse": "nerfh_coarse_lean_kernel"}


def _compile(tmp, name, *flags):
    """nerfh_mlp_lean.hip -> (assembly path, the compiler's resource remarks)"""
    out = os.path.join(tmp, name + ".s")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", *flags, os.path.join(CSRC, "nerfh_mlp_lean.hip"), "-o", out],
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


def _mnemonics(body):
    """{mnemonic: count} over a kernel's text (encoding suffixes _e32 / _e64 dropped)"""
    n = {}
    for raw in body:
        line = raw.split(";", 1)[0].strip()
        if not line or line.endswith(":") or line.startswith((".", "#")):
            continue
        op = re.sub(r"_(e32|e64|dpp|sdwa)$", "", line.split(None, 1)[0])
        n[op] = n.get(op, 0) + 1
    return n


def _kernels(path, remarks):
    rec = {}
    kind_of = lambda name: next((k for k, sub in KINDS.items() if sub in name), None)
    for r in mfma_free_valu.report(path):
        if kind_of(r["kernel"]):
            rec[kind_of(r["kernel"])] = r
    for name, body in mfma_free_valu.kernels(open(path).read().splitlines()):
        kind = kind_of(name)
        if kind:
            rec[kind]["read_distance"] = min(mfma_read_distance.scan(body)[1])
            rec[kind]["resources"] = next(v for k, v in _resources(remarks).items() if k == name)
            rec[kind]["ops"] = _mnemonics(body)
    assert set(rec) == {"fine", "coarse"}, sorted(rec)
    return rec


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """the two kernels of the unit as shipped"""
    rec = _kernels(*_compile(str(tmp_path_factory.mktemp("lean")), "lean"))
    for kind in ("fine", "coarse"):
        print(kind, {k: v for k, v in rec[kind].items() if k not in ("stretches40", "ops")},
              {op: rec[kind]["ops"].get(op, 0) for op in ("v_pk_max_u16", "v_pk_maximum3_f16", "v_rcp_iflag_f32", "v_mul_hi_u32",
                                                           "v_permlane32_swap_b32")})
    return rec


@pytest.mark.parametrize("kind,valu", (("fine", 3480), ("coarse", 2590)))
def test_vector_instructions(built, kind, valu):
    assert built[kind]["valu"] <= valu, built[kind]["valu"]


def test_the_select_chains_are_gone(built):
    f = built["fine"]
    assert f["writelane"] == 0
    assert f["cndmask"] + f["cmp"] <= 140, (f["cndmask"], f["cmp"])


@pytest.mark.parametrize("kind", ("fine", "coarse"))
def test_the_division_is_gone(built, kind):
    ops = built[kind]["ops"]
    assert ops.get("v_rcp_iflag_f32", 0) == 0, ops.get("v_rcp_iflag_f32")
    assert ops.get("v_mul_hi_u32", 0) >= 1   # the multiply-high that replaces it


@pytest.mark.parametrize("kind,left", (("fine", 8), ("coarse", 4)))
def test_the_range_guard_is_paired(built, kind, left):
    ops = built[kind]["ops"]
    assert ops.get("v_pk_max_u16", 0) <= left, ops.get("v_pk_max_u16")
    assert ops.get("v_pk_maximum3_f16", 0) >= 1


@pytest.mark.parametrize("kind,mfma", (("fine", 1920), ("coarse", 1560)))
def test_resources_and_mfma_counts(built, kind, mfma):
    k = built[kind]
    r = k["resources"]
    assert k["mfma"] == mfma
    assert r["VGPRs"] <= 256 and r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, r
    assert r["Occupancy [waves/SIMD]"] == 2, r
    assert k["read_distance"] >= 6, k["read_distance"]
    assert k["writelane"] == 0
