"""Distance, in MFMA issues, from the last MFMA that writes an accumulator register to the first inline-asm instruction that reads it,
for every such read of every kernel in a gfx950 assembly file (hipcc -save-temps: *-hip-amdgcn-amd-amdhsa-gfx950.s).  No GPU.

An XDL result read by an instruction inside inline asm is not interlocked (nerfh_mlp_core.h: layer()), so the conversion pieces of the
split-f16 kernels rely on the MFMAs that lie between producer and reader.  The scan is linear over each kernel's text (the layers are
straight-line code): every v_mfma marks its destination registers with its issue index; an instruction between #ASMSTART and #ASMEND
that names a marked register as a source gives one distance = MFMAs issued after the producer and before the reader; any other write
to a register clears its mark.

  python tools/mfma_read_distance.py file.s [kernel-name-substring ...]     one JSON line per kernel: reads, minimum, histogram
"""
import json
import re
import sys

REG = re.compile(r"\b([va])(\d+)\b|\b([va])\[(\d+):(\d+)\]")


def regs(operand):
    out = []
    for m in REG.finditer(operand):
        if m.group(1):
            out.append((m.group(1), int(m.group(2))))
        else:
            out.extend((m.group(3), i) for i in range(int(m.group(4)), int(m.group(5)) + 1))
    return out


def scan(lines):
    last, n_mfma, in_asm, dist = {}, 0, False, []
    for raw in lines:
        line = raw.split(";", 1)[0].strip() if "#ASM" not in raw else raw.strip()
        if "#ASMSTART" in line:
            in_asm = True
            continue
        if "#ASMEND" in line:
            in_asm = False
            continue
        if not line or line.endswith(":") or line.startswith("."):
            continue
        parts = line.split(None, 1)
        op, args = parts[0], (parts[1] if len(parts) > 1 else "")
        ops = [a.strip() for a in args.split(",")]
        if op.startswith("v_mfma"):
            for r in regs(ops[0]):
                last[r] = n_mfma
            n_mfma += 1
            continue
        if not (op.startswith("v_") or op.startswith("ds_") or op.startswith("global_") or op.startswith("buffer_") or op.startswith("scratch_")):
            continue
        stores = op.startswith(("ds_write", "ds_store", "global_store", "buffer_store", "scratch_store"))
        srcs = ops if stores else ops[1:]
        if in_asm:
            for o in srcs:
                for r in regs(o):
                    if r in last:
                        dist.append(n_mfma - last[r] - 1)
                        del last[r]   # the FIRST reader only
        if not stores:
            for r in regs(ops[0]):
                last.pop(r, None)
    return n_mfma, dist


def main():
    path, want = sys.argv[1], sys.argv[2:]
    text = open(path).read().splitlines()
    name, body = None, []
    for l in text:
        m = re.match(r"^(_Z\w+):", l)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if re.match(r"^\.Lfunc_end", l):
                if not want or any(w in name for w in want):
                    n, d = scan(body)
                    hist = {}
                    for x in d:
                        hist[x] = hist.get(x, 0) + 1
                    print(json.dumps(dict(kernel=name[:90], mfma=n, reads=len(d), minimum=min(d) if d else None,
                                          histogram={str(k): hist[k] for k in sorted(hist)[:6]})))
                name = None
            else:
                body.append(l)


if __name__ == "__main__":
    main()
