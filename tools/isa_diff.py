"""Are the gfx950 kernels of two device libraries the same, instruction for instruction?

    python3 tools/isa_diff.py OLD.so NEW.so [--rename OLDSYMBOL=NEWSYMBOL]...

For a change that must not touch the device code (a host-side refactor, a rename): build the library before and after with the same
`make device` and compare.  Every gfx950 code object of each library (tools/kernel_resources.py code_objects) is disassembled with
llvm-objdump and cut at the `<symbol>:` lines; the addresses and encodings objdump prints as trailing comments are dropped, so a
kernel may move to another translation unit, or sit at another offset of its code object, and still compare equal; for the same reason
the pc-relative literal behind an s_getpc_b64 (the address of a function or table in the same code object) is replaced by the symbol it
points at, and the padding behind a kernel is ignored.  Beside the text,
each kernel's entry in the AMDGPU metadata note is compared whole (registers, spills, LDS, scratch, kernel arguments, workgroup size).
A symbol that several code objects carry (a template two files instantiate) is compared as the sorted list of its copies.
--rename (repeatable): the kernel OLDSYMBOL of OLD.so is compared with NEWSYMBOL of NEW.so, without the `.name:` and `.symbol:` lines
of the metadata, which hold the symbol itself.

Prints the symbols that only one library has and the ones whose text or metadata differs, then one summary line; exit status 1 if
there was any difference."""
import re
import subprocess
import sys
import tempfile

from kernel_resources import READELF, code_objects

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def kernels(lib_path):
    """{symbol: sorted [(disassembly text, metadata text)]} over the gfx950 code objects of the library."""
    out = {}
    for blob in code_objects(lib_path):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob); f.flush()
            asm = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", f.name], capture_output=True, text=True, check=True).stdout
            notes = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
            syms = subprocess.run([OBJDUMP, "-t", f.name], capture_output=True, text=True, check=True).stdout
        meta = {}
        for block in notes.split("  - .agpr_count:")[1:]:
            block = block.split("\namdhsa.")[0]
            name = re.search(r"\.name:\s+(\S+)", block)
            if name:
                meta[name.group(1)] = block.strip()
        symbols = sorted((int(l.split()[0], 16), l.split()[-1]) for l in syms.splitlines() if re.match(r"[0-9a-f]{16} ", l) and len(l.split()) >= 4)
        sym, text, getpc = None, {}, None
        for line in asm.splitlines():
            m = re.match(r"<(.+)>:$", line)
            if m:
                sym = m.group(1); text[sym] = []
                continue
            ins, _, comment = line.partition("//")
            ins = ins.rstrip()
            if sym is None or not ins.strip() or ins.strip() == "...":
                continue
            m = re.match(r"\s*s_add_u32 (s\d+), \1, (0x[0-9a-f]+|-?\d+)$", ins) if getpc is not None else None
            if m:      # s_getpc_b64 gives the address behind itself; the literal is relative to that
                off = int(m.group(2), 0)
                target = getpc + 4 + (off - (1 << 32) if off >= (1 << 31) else off)
                below = [(a, n) for a, n in symbols if a <= target]
                if below:
                    ins = "%s<%s+0x%x>" % (ins[:ins.rindex(m.group(2))], below[-1][1], target - below[-1][0])
            getpc = int(comment.split(":")[0], 16) if "s_getpc_b64" in ins else None
            text[sym].append(ins)
        for s, lines in text.items():
            out.setdefault(s, []).append(("\n".join(lines), meta.get(s, "")))
    return {s: sorted(v) for s, v in out.items()}


def main(old_path, new_path, renames=()):
    old, new = kernels(old_path), kernels(new_path)
    for o, n in renames:
        if o in old and n in new and n not in old:
            nameless = lambda v, s: sorted((t, re.sub(r"^\s*\.(name|symbol):\s+%s(\.kd)?\n" % re.escape(s), "", m, flags=re.M)) for t, m in v)
            old[n], new[n] = nameless(old.pop(o), o), nameless(new[n], n)
    bad = 0
    for s in sorted(set(old) - set(new)):
        print("only in %s: %s" % (old_path, s)); bad += 1
    for s in sorted(set(new) - set(old)):
        print("only in %s: %s" % (new_path, s)); bad += 1
    for s in sorted(set(old) & set(new)):
        a, b = old[s], new[s]
        if a == b:
            continue
        bad += 1
        what = []
        if [t for t, _ in a] != [t for t, _ in b]:
            what.append("text")
        if [m for _, m in a] != [m for _, m in b]:
            what.append("metadata")
        print("differs (%s): %s" % (" and ".join(what), s))
    print("isa_diff: %d symbols compared, %d differ or are missing" % (len(set(old) | set(new)), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    renames = []
    while "--rename" in args[:-1]:
        i = args.index("--rename")
        renames.append(tuple(args[i + 1].split("=", 1)))
        del args[i:i + 2]
    if len(args) != 2 or any(len(r) != 2 for r in renames):
        sys.exit(__doc__)
    sys.exit(main(args[0], args[1], renames))
