"""Kernel-by-kernel comparison of device assembly (runs here, no GPU): every kernel of the OLD files must exist exactly once, under the
same demangled name, in the NEW files, with the same instruction sequence and the same resource metadata.  Text only: local labels are
renumbered in order of first appearance and symbol names (which carry the translation unit's hash for internal linkage) are replaced by
their demangled form; nothing else is interpreted.
usage: python scripts/asm_diff_kernels.py OLD.s[,OLD2.s...] NEW.s[,NEW2.s...] [name-filter-regex]
       (the .s files: hipcc <build.py's flags> -S --cuda-device-only UNIT.hip -o UNIT.s)
Prints one line per kernel of OLD, "identical" or the first differing line; exit status 1 if any kernel differs, is missing or doubled."""
import re, subprocess, sys

META = ("sgpr_count", "vgpr_count", "agpr_count", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "kernarg_segment_size", "max_flat_workgroup_size", "wavefront_size", "uses_dynamic_stack")
COMMENT_META = ("Occupancy", "LDSByteSize", "ScratchSize", "NumVgprs", "NumAgprs", "NumSgprs", "TotalNumSgprs", "codeLenInByte")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(anonymous namespace\)::", "", d) for n, d in zip(names, out)}


def kernels(path):
    """demangled name -> (normalised instruction lines, metadata dict), for every kernel (.amdhsa_kernel) of the file"""
    lines = open(path).read().split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    syms = sorted(set(re.findall(r"\b_Z\w+", "\n".join(lines))), key=len, reverse=True)
    dem = demangle(syms)
    meta = {}
    entry = {}
    for l in lines + ["  - ."]:           # the metadata block at the end of the file: one list entry per kernel, its own keys at indentation 4
        if l.startswith("  - ."):
            if entry.get("name") in names: meta[entry["name"]] = {"." + k: v for k, v in entry.items() if k in META}
            entry = {}
        m = re.match(r"  [ -] \.(\w+):\s+(\S+)", l)
        if m: entry[m.group(1)] = m.group(2)
    out = {}
    for n in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(n + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        labels, body, md = {}, [], dict(meta.get(n, {}))
        for l in lines[start + 1:end]:
            t = l.split(";")[0].strip() if not l.strip().startswith(";") else ""
            if t.startswith(".amdhsa_") and not t.startswith(".amdhsa_kernel"): md[t.split()[0]] = t.split()[1]        # the kernel descriptor
            if not t or t.startswith(".") and not t.endswith(":"): continue          # comments and directives
            body.append(t)
        text = "\n".join(body)
        for lab in re.findall(r"\.L\w+", text):
            labels.setdefault(lab, ".L%d" % len(labels))
        text = re.sub(r"\.L\w+", lambda m: labels[m.group(0)], text)
        text = re.sub(r"\b_Z\w+", lambda m: dem.get(m.group(0), m.group(0)), text)
        for l in lines[end:end + 120]:                                                # the compiler's comment block behind the function
            m = re.match(r";\s*(\w+)\s*[:=]\s*(\S+)", l)
            if m and m.group(1) in COMMENT_META and m.group(1) not in md: md[m.group(1)] = m.group(2)
            if l.strip().startswith(".amdhsa_kernel") or (l.endswith(":") and not l.startswith((".", ";"))): break
        out.setdefault(dem.get(n, n), []).append((text.split("\n"), md))          # (a kernel declared extern "C" has no mangled name)
    return out


def merged(paths):
    all_ = {}
    for p in paths.split(","):
        for k, v in kernels(p).items(): all_.setdefault(k, []).extend(v)
    return all_


old, new = merged(sys.argv[1]), merged(sys.argv[2])
want = re.compile(sys.argv[3]) if len(sys.argv) > 3 else None
bad = 0
for name in sorted(old):
    if want and not want.search(name): continue
    (a, ma), = old[name]
    short = name if len(name) <= 110 else name[:107] + "..."
    if len(new.get(name, [])) != 1:
        print("%-112s %s in the new files" % (short, "MISSING" if name not in new else "%d copies" % len(new[name]))); bad += 1; continue
    (b, mb), = new[name]
    diff = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None if len(a) == len(b) else min(len(a), len(b)))
    if diff is not None:
        print("%-112s DIFFERS at instruction %d of %d / %d:\n    old: %s\n    new: %s" % (short, diff, len(a), len(b), a[diff] if diff < len(a) else "<end>", b[diff] if diff < len(b) else "<end>")); bad += 1
    elif ma != mb:
        print("%-112s instructions identical, METADATA differs: %s" % (short, ", ".join("%s %s -> %s" % (k, ma.get(k), mb.get(k)) for k in sorted(set(ma) | set(mb)) if ma.get(k) != mb.get(k)))); bad += 1
    else:
        print("%-112s identical (%d instructions; VGPR %s AGPR %s SGPR %s LDS %s scratch %s occupancy %s)" % (short, len(a), ma.get(".vgpr_count"), ma.get(".agpr_count"), ma.get(".sgpr_count"),
              ma.get(".group_segment_fixed_size"), ma.get(".private_segment_fixed_size"), ma.get("Occupancy")))
extra = sorted(k for k in new if k not in old and (not want or want.search(k)))
for k in extra: print("%-112s only in the new files" % (k if len(k) <= 110 else k[:107] + "..."))
sys.exit(1 if bad else 0)
