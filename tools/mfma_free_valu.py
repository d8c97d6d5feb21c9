"""Vector instructions that no MFMA covers, for every kernel in a gfx950 assembly file (hipcc -O3 -S --cuda-device-only, or the
*-hip-amdgcn-amd-amdhsa-gfx950.s of -save-temps).  No GPU.

The split-f16 render kernels keep the matrix pipe busy only while MFMAs are in flight; vector instructions that stand between two
v_mfma are partly hidden in the MFMAs' shadow, those in a long stretch without any are not (LABBOOK R18.1, R19.1: such stretches cost
two to three times the average slope).  The scan is linear over each kernel's text, as tools/mfma_read_distance.py's: every
instruction whose mnemonic starts with v_ and is no v_mfma counts as one vector instruction; a stretch is the run of them between two
consecutive v_mfma (the head in front of the first and the tail behind the last included; the tile loop's text is straight-line code).

  python tools/mfma_free_valu.py file.s [kernel-name-substring ...]
      one JSON line per kernel: mfma, valu, readlane / writelane / cndmask / cmp, the six longest stretches as [length, MFMAs in
      front of it], and free40 = the sum over the stretches of 40 or more
"""
import json
import re
import sys

LONG = 40   # a stretch this long has left every MFMA's shadow (16 passes x 4 cycles of the 16x16x32 MFMA in front of it at the most)


def scan(lines):
    """(MFMAs, vector instructions, {class: count}, [(length, MFMAs in front)] for every stretch, in text order)"""
    n_mfma, n_valu, run = 0, 0, 0
    kinds = dict(readlane=0, writelane=0, cndmask=0, cmp=0)
    stretches = []
    for raw in lines:
        line = raw.split(";", 1)[0].strip()
        if not line or line.endswith(":") or line.startswith((".", "#")):
            continue
        op = line.split(None, 1)[0]
        if op.startswith("v_mfma"):
            stretches.append((run, n_mfma))
            run = 0
            n_mfma += 1
            continue
        if not op.startswith("v_"):
            continue
        n_valu += 1
        run += 1
        if op.startswith("v_readlane"):
            kinds["readlane"] += 1
        elif op.startswith("v_writelane"):
            kinds["writelane"] += 1
        elif op.startswith("v_cndmask"):
            kinds["cndmask"] += 1
        elif op.startswith("v_cmp"):   # v_cmp_* and v_cmpx_*
            kinds["cmp"] += 1
    stretches.append((run, n_mfma))
    return n_mfma, n_valu, kinds, stretches


def kernels(text):
    """(name, body lines) of every function of the file"""
    name, body = None, []
    for l in text:
        m = re.match(r"^(_Z\w+):", l)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r"^\.Lfunc_end", l):
                yield name, body
                name = None
            else:
                body.append(l)


def report(path, want=()):
    """one dict per kernel of `path` whose name holds one of `want` (all of them if empty)"""
    out = []
    for name, body in kernels(open(path).read().splitlines()):
        if want and not any(w in name for w in want):
            continue
        n_mfma, n_valu, kinds, stretches = scan(body)
        longest = sorted(stretches, key=lambda s: -s[0])[:6]
        out.append(dict(kernel=name[:90], mfma=n_mfma, valu=n_valu, **kinds, longest=[list(s) for s in longest],
                        free40=sum(s[0] for s in stretches if s[0] >= LONG),
                        stretches40=[list(s) for s in stretches if s[0] >= LONG]))
    return out


def main():
    for rec in report(sys.argv[1], sys.argv[2:]):
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
