"""Compare the gfx950 instruction streams of two builds, kernel by kernel:

    python -m mkb_amd.csrc.build --force --save-temps      # in each tree: leaves *-gfx950.s in mkb_amd/csrc/_obj
    python tools/kernel_asm_diff.py OLD_DIR NEW_DIR [--map old_symbol=new_symbol ...]

Functions are matched by symbol across all files of a directory (a kernel may have moved to another translation unit); comments,
directives and blank lines are dropped and local labels lose their function number.  One line per symbol: identical, or differs
with both instruction counts and whether the multiset of opcodes is equal, or the build it is missing from.  It is a diff: it
judges nothing.  Symbols are cut to 110 characters in the output."""
import argparse
import collections
import pathlib
import re

START = re.compile(r"^([A-Za-z_$][\w$.]*):\s*(;.*)?$")  # a function's label (local labels begin with .L)
LOCAL = re.compile(r"\.L(BB|tmp|func_begin)\d+_")


def kernels(directory):
    """symbol -> (file stem, [instruction and label lines])"""
    out = {}
    for path in sorted(pathlib.Path(directory).glob("*-gfx950.s")):
        name, body = None, []
        for line in path.read_text().splitlines():
            if name is None:
                m = START.match(line)
                if m:
                    name, body = m.group(1), []
            elif line.startswith(".Lfunc_end"):
                out[name] = (path.name.split("-hip-")[0], body)
                name = None
            else:
                code = LOCAL.sub(r".L\1_", line.split(";")[0].strip())
                if code and (not code.startswith(".") or code.endswith(":")):
                    body.append(code)
    return out


def opcodes(body):
    return collections.Counter(line.split()[0] for line in body if not line.endswith(":"))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old_dir")
    ap.add_argument("new_dir")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW", help="a kernel that was renamed")
    args = ap.parse_args()
    old, new = kernels(args.old_dir), kernels(args.new_dir)
    renamed = dict(m.split("=", 1) for m in args.map)
    short = lambda sym: sym[:110] + ("..." if len(sym) > 110 else "")
    tally = collections.Counter()
    for sym, (f_old, a) in sorted(old.items()):
        to = renamed.get(sym, sym)
        f_new, b = new.get(to, (None, None))
        if b is None:
            kind, what = "only in old", f"only in old ({sum(opcodes(a).values())} instructions)"
        elif a == b:
            kind = what = "identical"
        else:
            kind = "differs"
            what = (f"differs: {sum(opcodes(a).values())} -> {sum(opcodes(b).values())} instructions, opcode multiset "
                    f"{'equal' if opcodes(a) == opcodes(b) else 'differs'}")
        if f_new not in (None, f_old):
            what += f"  [{f_old} -> {f_new}]"
        tally[kind] += 1
        print(f"{f_old:20s} {short(sym)}{' -> ' + short(to) if to != sym else ''}: {what}")
    for sym in sorted(set(new) - {renamed.get(s, s) for s in old}):
        tally["only in new"] += 1
        print(f"{new[sym][0]:20s} {short(sym)}: only in new ({sum(opcodes(new[sym][1]).values())} instructions)")
    print("\n" + ", ".join(f"{n} {kind}" for kind, n in sorted(tally.items())))


if __name__ == "__main__":
    main()
