#!/usr/bin/env python3
"""Dev tool (CPU): compare the kernels of two device-assembly files of the API translation unit, kernel by kernel.

    python tools/asm_compare.py OLD.s NEW.s [--rename MAP] [--filter REGEX]

OLD.s / NEW.s: the output of the hipcc line in tools/kernel_resources.sh (--cuda-device-only -S), one per tree.
MAP: a text file, one "old new" pair per line ('#' starts a comment): kernels whose name changed between the trees.  A name
is a mangled kernel name, or a regular expression over it with the replacement in re.sub syntax when the line starts with
"re:" (re: <pattern> <replacement>), so that one line maps a whole family of instantiations.

Per kernel it says whether the instruction stream is identical -- the text between the kernel's label and its descriptor,
comments dropped, local labels numbered in order of appearance, the kernel's own name (and the renamed names) normalised --
and whether the kernel descriptor is: the .amdhsa_ directives and the resource fields of the code-object metadata (registers,
spills, LDS, scratch, kernel-argument size).  For a kernel that differs it prints the instruction counts and the descriptor
fields that differ.  Kernels in one file only are listed as removed / new.  It compares text; it knows no instruction.
Exit status 0; the verdict is the output.
"""
import argparse
import re
import sys

META_FIELDS = ("agpr_count", "vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
               "group_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size")


def parse(path):
    """{kernel: (body lines, {descriptor field: value})} of one assembly file, in file order."""
    lines = open(path).read().split("\n")
    kernels = {}
    i, n = 0, len(lines)
    while i < n:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if not m:
            i += 1
            continue
        name = m.group(1)
        desc = {}
        j = i + 1
        while not lines[j].strip().startswith(".end_amdhsa_kernel"):
            parts = lines[j].split(";")[0].split()
            if len(parts) == 2:
                desc[parts[0]] = parts[1]
            j += 1
        # the body: back from the descriptor to the kernel's label
        k = i
        while k >= 0 and not lines[k].startswith(name + ":"):
            k -= 1
        body = []
        for ln in lines[k + 1:i]:
            ln = ln.split(";")[0].strip()
            if ln and not ln.startswith((".section", ".p2align")):
                body.append(ln)
        kernels[name] = (body, desc)
        i = j + 1
    # resource fields of the metadata: entries of amdhsa.kernels, scalars at the entry's own indentation
    def flush(entry):
        if entry and entry.get("name") in kernels:
            kernels[entry["name"]][1].update((f, entry[f]) for f in META_FIELDS if f in entry)

    cur = None
    inmeta = False
    for ln in lines:
        if ln.strip() == ".amdgpu_metadata":
            inmeta = True
        elif ln.strip() == ".end_amdgpu_metadata":
            inmeta = False
            flush(cur)
            cur = None
        if not inmeta:
            continue
        if ln.startswith("  - "):
            flush(cur)
            cur = {}
            ln = "    " + ln[4:]
        m = re.match(r"    \.(\w+):\s*(\S+)\s*$", ln)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return kernels


def load_map(path):
    plain, rules = {}, []
    if path:
        for ln in open(path):
            ln = ln.split("#")[0].split()
            if not ln:
                continue
            if ln[0] == "re:":
                rules.append((re.compile(ln[1]), ln[2]))
            else:
                plain[ln[0]] = ln[1]
    return plain, rules


def renamed(name, plain, rules):
    if name in plain:
        return plain[name]
    for pat, rep in rules:
        if pat.fullmatch(name):
            return pat.sub(rep, name)
    return name


def normalise(body, names):
    """names: {symbol: token}; the mangled name also occurs without its _Z inside the names of function-local symbols."""
    out, labels = [], {}
    subs = sorted(((s[2:] if s.startswith("_Z") else s, t) for s, t in names.items()), key=lambda p: -len(p[0]))

    def lab(m):
        return labels.setdefault(m.group(0), ".L%d" % len(labels))

    for ln in body:
        for s, t in subs:
            if s in ln:
                ln = ln.replace(s, t)
        out.append(re.sub(r"\.L[A-Za-z_]+\d+(?:_\d+)?", lab, ln))
    return out


def count(body):
    return sum(1 for ln in body if not ln.endswith(":") and not ln.startswith("."))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", default=None)
    ap.add_argument("--filter", default="", help="only kernels whose (old) name matches")
    a = ap.parse_args()
    old, new = parse(a.old), parse(a.new)
    plain, rules = load_map(a.rename)
    pairs = {o: renamed(o, plain, rules) for o in old}
    names = {}
    for o, nn in pairs.items():                      # a renamed kernel is one symbol, whichever file names it
        names[o] = names[nn] = "<%d>" % len(names)
    same = differ = 0
    matched = set()
    for o, (obody, odesc) in old.items():
        if a.filter and not re.search(a.filter, o):
            continue
        nn = pairs[o]
        if nn not in new:
            print("removed kernel: %s%s" % (o, "" if nn == o else "  (renamed to %s: not in %s)" % (nn, a.new)))
            continue
        matched.add(nn)
        nbody, ndesc = new[nn]
        code = normalise(obody, names) == normalise(nbody, names)
        desc = odesc == ndesc
        tag = nn if nn == o else "%s  <-  %s" % (nn, o)
        print("instruction stream %s, kernel descriptor %s: %s" % ("identical" if code else "different",
                                                                    "identical" if desc else "different", tag))
        same += code and desc
        differ += not (code and desc)
        if not code:
            print("    instructions: %d  <-  %d" % (count(nbody), count(obody)))
        if not code or not desc:
            keys = [k for k in sorted(set(odesc) | set(ndesc)) if odesc.get(k) != ndesc.get(k)]
            print("    descriptor fields that differ: %s" % (", ".join("%s %s <- %s" % (k.replace(".amdhsa_", ""), ndesc.get(k), odesc.get(k))
                                                                       for k in keys) or "none"))
            print("    " + " ".join("%s %s" % (f, ndesc.get(f)) for f in META_FIELDS[:8]))
    extra = [k for k in new if k not in matched and not (a.filter and not re.search(a.filter, k))]
    for k in extra:
        print("new kernel: %s" % k)
    print("identical %d different %d removed %d new %d" % (same, differ, sum(1 for o in old if pairs[o] not in new and
                                                                          not (a.filter and not re.search(a.filter, o))), len(extra)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
