"""Static instruction counts of the packet kernel's slim instantiations, for the diet of round 24 (packetkernel.hip DIET).

    python3 tools/diet_isa.py [-DPT_PK_NO_DIET_NODE] > listing      (runs hipcc -S as tools/node_step_isa.py does; no GPU needed)

Per kernel: the whole body; the node step (from the inner loop's header in front of the first v_min_f64 -- the mask of the lanes at a
node, the gathers, the slab tests, the key sort, the branch-free tail -- to the s_branch behind that tail); the whole node loop (every
block the listing attributes to that inner loop: the step, the branched tail for a stack nearly full or spilled to HBM, the loop's exec
bookkeeping) -- each as vector / scalar / LDS / gather counts; and the idioms the diet is about: 0 / 1 selects that feed a compare
with 0 (a ballot through an int), canonicalising v_max_f32 x, x, and v_sqrt_f32."""
import collections, os, re, subprocess, sys, tempfile
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assembly(src, flags):
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "pk.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", "-fPIC", "-ffp-contract=off"] + flags + ["-include", "cstring",
                               "-I" + os.path.join(REPO, "include"), "-S", "--cuda-device-only", os.path.join(REPO, "minimaloptix_amd", "csrc", src), "-o", asm],
                              stderr=subprocess.DEVNULL)
        return open(asm).read().split("\n")


def ops(lines):
    return [m.group(1) for m in (re.match(r"\s+([a-z][a-z_0-9]+)\s", l + " ") for l in lines) if m and not m.group(1).startswith("s_nop")]


def counts(lines):
    c = collections.Counter(ops(lines))
    pick = lambda p: sum(n for k, n in c.items() if k.startswith(p))
    return "vector %4d  scalar %4d  LDS %3d  gathers %3d" % (pick("v_"), pick("s_"), pick("ds_"), pick("global_load"))


def idioms(lines):
    sel = sum(1 for i, l in enumerate(lines) if re.match(r"\s+v_cndmask_b32_e64 (v\d+), 0, 1,", l) and
              any(re.match(r"\s+v_cmp_ne_u32\S* .*\b0, %s$" % re.match(r"\s+v_cndmask_b32_e64 (v\d+)", l).group(1), x) for x in lines[i + 1:i + 6]))
    canon = sum(1 for l in lines if re.match(r"\s+v_max_f32_e32 v\d+, (v\d+), \1$", l))
    sqrt = sum(1 for l in lines if re.match(r"\s+v_sqrt_f32", l))
    return "ballot through an int (0/1 select + compare) %d, canonicalising v_max_f32 x, x %d, v_sqrt_f32 %d" % (sel, canon, sqrt)


def main(extra):
    asm = {"1": assembly("packetkernel.hip", ["-mllvm", "-amdgpu-sched-strategy=max-ilp"] + extra), "0": assembly("packetkernel_n128.hip", extra)}
    print("flags: %s" % (" ".join(extra) or "(none: the tree as it builds)"))
    for near in ("0", "1"):
        for n64 in ("1", "0"):
            name = "_ZN2pt12_GLOBAL__N_115pt_packetkernelILb0ELb1ELb0ELb%sELb%sEEEvNS_10LaunchArgsE" % (near, n64)
            txt = asm[n64]
            start = [i for i, l in enumerate(txt) if l.startswith(name + ":")][0]
            end = [i for i, l in enumerate(txt) if i > start and l.startswith(".Lfunc_end")][0]
            body = txt[start:end]
            print("== pt_packetkernel<false,true,false,%s,%s>%s" % ("true" if near == "1" else "false", "true" if n64 == "1" else "false",
                                                                    "   (the benchmark's kernel)" if (near, n64) == ("0", "1") else ""))
            print("   whole kernel    %s" % counts(body))
            print("   idioms          %s" % idioms(body))
            first = [i for i, l in enumerate(body) if "v_min_f64" in l][0]
            lo = first
            while "Inner Loop Header" not in body[lo]: lo -= 1
            hi = first
            while "s_branch" not in body[hi]: hi += 1
            print("   node step       %s      | %s" % (counts(body[lo:hi + 1]), idioms(body[lo:hi + 1])))
            hdr = re.search(r"LBB\d+_\d+", body[lo - 1]).group(0)
            last = max(i for i, l in enumerate(body) if re.search(r"Header=%s\b" % hdr[1:], l))
            stop = last + 1
            while not re.match(r"\.LBB|; %bb", body[stop]): stop += 1      # the end of the loop's last block
            print("   node loop       %s" % counts(body[lo:stop]))


if __name__ == "__main__":
    main(sys.argv[1:])
