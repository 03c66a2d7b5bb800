#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel (no GPU needed).

Each directory holds the `.s` files of `hipcc $(CXXFLAGS) --cuda-device-only -S pam_X.hip -o DIR/pam_X.s` (Makefile flags; once more
with -DPAM_DIAG for the diagnostic build).  Per kernel the body (symbol to .Lfunc_end), the .amdhsa_kernel descriptor and the
kernel's .amdgpu_metadata entry must be equal after three normalisations: assembler comments dropped, the random __hip_cuid_* symbol, and local labels
(.LBB / .Lfunc_end / .Ltmp), renumbered in order of appearance because their function index moves with definition order.
Kernels are pooled by symbol over all files of a directory, so a kernel that moved to another source file is still compared; the
report names the file(s) it sits in.
usage: device_code_diff.py OLD_DIR NEW_DIR [--explain]     exit status 1 when a kernel differs or exists on one side only
--explain: under every kernel that differs, the instruction count of each side, the mnemonics whose counts changed and the descriptor /
metadata lines that changed -- what a restructured kernel is judged by (tools/README.md).
"""
import collections
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


def pool(directory):
    """symbol -> (file name, [body, descriptor, metadata]) over every .s file of the directory; a symbol defined in two files is an error."""
    out = {}
    for path in sorted(pathlib.Path(directory).glob("*.s")):
        for k, parts in kernels(path).items():
            if k in out:
                sys.exit("%s: %s is defined in %s and %s" % (directory, k, out[k][0], path.name))
            out[k] = (path.name, parts)
    return out


def mnemonics(body):
    """Counter of instruction mnemonics of a normalised body (labels and directives are no instructions)."""
    words = (l.split()[0] for l in body.splitlines() if l.strip())
    return collections.Counter(w for w in words if not w.endswith(":") and not w.startswith("."))


def explain(old, new):
    """Lines for one differing kernel: [body, descriptor, metadata] of each side."""
    a, b = mnemonics(old[0]), mnemonics(new[0])
    out = ["    instructions: %d -> %d" % (sum(a.values()), sum(b.values()))]
    moved = ["%s %d -> %d" % (m, a[m], b[m]) for m in sorted(a.keys() | b.keys()) if a[m] != b[m]]
    out.append("    mnemonic counts: " + (", ".join(moved) if moved else "all equal (order or registers only)"))
    for part, x, y in (("descriptor", old[1], new[1]), ("metadata", old[2], new[2])):
        xs, ys = x.splitlines(), y.splitlines()
        for l in [l for l in xs if l not in ys]:
            out.append("    %s old: %s" % (part, l.strip()))
        for l in [l for l in ys if l not in xs]:
            out.append("    %s new: %s" % (part, l.strip()))
    return out


def main(old_dir, new_dir, verbose=False):
    a, b = pool(old_dir), pool(new_dir)
    bad = 0
    for k in sorted(a.keys() | b.keys()):
        where = " / ".join(sorted({d[k][0] for d in (a, b) if k in d}))
        if k not in a or k not in b:
            bad += 1
            print("%s: %s only in %s" % (where, k, "old" if k in a else "new"))
        elif a[k][1] != b[k][1]:
            bad += 1
            print("%s: %s differs (%s)" % (where, k, ", ".join(p for p, x, y in zip(("body", "descriptor", "metadata"), a[k][1], b[k][1]) if x != y)))
            if verbose:
                print("\n".join(explain(a[k][1], b[k][1])))
    print("%d kernels in old, %d in new, %d compared, %d differ" % (len(a), len(b), len(a.keys() | b.keys()), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    dirs = [x for x in sys.argv[1:] if x != "--explain"]
    sys.exit(main(dirs[0], dirs[1], "--explain" in sys.argv[1:]))
