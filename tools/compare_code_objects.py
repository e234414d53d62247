#!/usr/bin/env python3
"""Are the gfx950 kernels of two builds the same code?  The proof a refactor of device code needs, on a machine without a GPU.

    python tools/compare_code_objects.py A.so B.so

Extracts the gfx950 code objects of both libraries (`llvm-objdump --offloading`) and compares, per kernel symbol, the instruction stream
(mnemonic, operands and encoding; addresses dropped, branch targets as labels) and the 64-byte kernel descriptor (its code entry offset
excluded: the same kernels may sit at other addresses).  Prints kernels / instructions / differences and exits non-zero on any difference or
when the two symbol sets differ.  The files themselves need not be byte-identical: templates instantiated in another order land elsewhere.
"""
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-wavenet_amd"))
import build as wn_build  # noqa: E402

ENTRY_OFFSET = slice(16, 24)   # kernel_code_entry_byte_offset of the 64-byte descriptor


def kernels(so, objdump):
    """{kernel symbol: (instructions, descriptor bytes)} over every gfx950 code object of `so`; an instruction is (text, encoding)."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        local = shutil.copy(so, os.path.join(tmp, "lib.so"))
        subprocess.check_call([objdump, "--offloading", local], cwd=tmp, stdout=subprocess.DEVNULL)
        objs = sorted(f for f in os.listdir(tmp) if "gfx950" in f)
        if not objs:
            raise SystemExit("%s: no gfx950 code object" % so)
        for co in objs:
            path = os.path.join(tmp, co)
            # the descriptors: objects <kernel>.kd in .rodata
            syms = subprocess.check_output([objdump, "-t", path]).decode()
            kds = {}
            for line in syms.splitlines():
                m = re.match(r"^([0-9a-f]+)\s.*\s\.rodata\s+([0-9a-f]+)\s+(?:\.\w+\s+)?(\S+)\.kd$", line)
                if m and int(m.group(2), 16) == 64:
                    kds[m.group(3)] = int(m.group(1), 16)
            rodata = subprocess.check_output([objdump, "-s", "-j", ".rodata", path]).decode()
            mem = {}
            for line in rodata.splitlines():
                m = re.match(r"^ ([0-9a-f]+) ((?:[0-9a-f]+ ?)+) ", line)
                if m:
                    base = int(m.group(1), 16)
                    for i, b in enumerate(bytes.fromhex(m.group(2).replace(" ", ""))):
                        mem[base + i] = b
            dis = subprocess.check_output([objdump, "-d", "--symbolize-operands", path]).decode()
            cur, labels = None, {}
            for line in dis.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    if re.fullmatch(r"L\d+", m.group(1)):   # a branch target: numbered per kernel, in address order
                        if cur:
                            out[cur][0].append(("label %d" % labels.setdefault(m.group(1), len(labels)), ""))
                        continue
                    cur, labels = m.group(1), {}
                    if cur in out:
                        raise SystemExit("%s: kernel symbol %s in two code objects" % (so, cur))
                    out[cur] = ([], None)
                    continue
                if not cur or "//" not in line:
                    continue
                text, _, tail = line.partition("//")
                enc = tail.split(":", 1)[1].split() if ":" in tail else []   # "// 0000000012A4: BF8C0F70" -> the encoding words
                text = re.sub(r"\bL\d+\b", lambda k: "L#%d" % labels.setdefault(k.group(0), len(labels)), text.strip())
                out[cur][0].append((text, " ".join(enc)))
            for k in [k for k in out if out[k][1] is None]:
                if k not in kds:
                    del out[k]   # a device function that was not inlined: no kernel
                    continue
                kd = bytearray(mem[kds[k] + i] for i in range(64))
                kd[ENTRY_OFFSET] = bytes(8)
                out[k] = (out[k][0], bytes(kd))
    return out


def main(argv):
    if len(argv) != 3:
        raise SystemExit(__doc__)
    objdump = wn_build.objdump_path()
    a, b = kernels(argv[1], objdump), kernels(argv[2], objdump)
    diffs = 0
    for name, which in [(n, "first") for n in sorted(set(a) - set(b))] + [(n, "second") for n in sorted(set(b) - set(a))]:
        print("only in the %s library: %s" % (which, name))
        diffs += 1
    n_ins = 0
    for k in sorted(set(a) & set(b)):
        (ia, da), (ib, db) = a[k], b[k]
        n_ins += len(ia)
        if da != db:
            print("%s: kernel descriptors differ\n    %s\n    %s" % (k, da.hex(), db.hex()))
            diffs += 1
        if ia != ib:
            diffs += 1
            at = next((i for i, (x, y) in enumerate(zip(ia, ib)) if x != y), min(len(ia), len(ib)))
            print("%s: %d / %d instructions, first difference at instruction %d\n    %r\n    %r" % (
                k, len(ia), len(ib), at, ia[at] if at < len(ia) else None, ib[at] if at < len(ib) else None))
    print("%d kernels compared, %d instructions, %d differences" % (len(set(a) & set(b)), n_ins, diffs))
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
