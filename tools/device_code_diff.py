#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel (no GPU needed).

Each directory holds the `.s` files of `hipcc $(CXXFLAGS) --cuda-device-only -S pam_X.hip -o DIR/pam_X.s` (Makefile flags; once more
with -DPAM_DIAG for the diagnostic build).  Per kernel the body (symbol to .Lfunc_end), the .amdhsa_kernel descriptor and the
kernel's .amdgpu_metadata entry must be equal after three normalisations: assembler comments dropped, the random __hip_cuid_* symbol, and local labels
(.LBB / .Lfunc_end / .Ltmp), renumbered in order of appearance because their function index moves with definition order.
usage: device_code_diff.py OLD_DIR NEW_DIR      exit status 1 when a kernel differs or exists on one side only
"""
import pathlib
import re
import sys

CUID = re.compile(r"__hip_cuid_\w+")
LABEL = re.compile(r"\.L(?:BB|func_end|tmp)[0-9_]+")
COMMENT = re.compile(r"[ \t]*;.*$", re.M)


def norm(lines):
    seen = {}
    # assembler comments go first: they name basic blocks by their function-wide number (";   in Loop: Header=BB166_5"), which moves
    # whenever an instantiation is added in front of the kernel, like the labels
    text = CUID.sub("__hip_cuid_X", "".join(COMMENT.sub("", l) for l in lines))
    return LABEL.sub(lambda m: seen.setdefault(m.group(0), ".L%d" % len(seen)), text)


def kernels(path):
    lines = path.read_text().splitlines(keepends=True)
    desc = {l.split()[1]: i for i, l in enumerate(lines) if l.lstrip().startswith(".amdhsa_kernel ")}
    label = {l.split(":")[0]: i for i, l in enumerate(lines) if not l[:1].isspace() and ":" in l}
    out = {}
    for k, d0 in desc.items():
        start = label[k]
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        d1 = next(i for i in range(d0, len(lines)) if ".end_amdhsa_kernel" in lines[i])
        out[k] = [norm(lines[start:end]), norm(lines[d0:d1])]
    meta = "".join(lines[next(i for i, l in enumerate(lines) if l.strip() == ".amdgpu_metadata"):])
    meta = meta.split("\namdhsa.target:")[0]          # the file's trailer is no part of the last kernel's entry
    for entry in re.split(r"\n  - (?=\.)", meta)[1:]:
        name = re.search(r"^    \.name:\s+(\S+)", entry, re.M).group(1)
        out[name].append(norm([entry]))
    return out


def main(old_dir, new_dir):
    total = bad = 0
    for old in sorted(pathlib.Path(old_dir).glob("*.s")):
        a, b = kernels(old), kernels(pathlib.Path(new_dir) / old.name)
        for k in sorted(a.keys() | b.keys()):
            total += 1
            if k not in a or k not in b:
                bad += 1
                print("%s: %s only in %s" % (old.name, k, "old" if k in a else "new"))
            elif a[k] != b[k]:
                bad += 1
                print("%s: %s differs (%s)" % (old.name, k, ", ".join(p for p, x, y in zip(("body", "descriptor", "metadata"), a[k], b[k]) if x != y)))
    print("%d kernels compared, %d differ" % (total, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
