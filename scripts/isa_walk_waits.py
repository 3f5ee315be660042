"""Development aid: two questions about `hipcc -S` listings of the kernels that walk rows with pl_median3_rows.
    python scripts/isa_walk_waits.py waits file.s kernel-name-fragment ...   s_waitcnt vmcnt(N) by N inside the kernel's LARGEST
                                                                            loop (the rolled row walk), and in the whole kernel
    python scripts/isa_walk_waits.py same a.s b.s                           kernel by kernel: are the instructions of a.s and
                                                                            b.s equal (labels, comments and directives aside)"""
import collections
import re
import sys


def kernels(path):
    """{kernel symbol: [instruction lines]} of every function of the listing"""
    s = open(path).read()
    out = {}
    for m in re.finditer(r"^([A-Za-z_]\w*):\s*(?:;.*)?$", s, re.M):
        k = s.find(".Lfunc_end", m.end())
        if k < 0:
            continue
        body = []
        for line in s[m.end():k].split("\n"):
            line = line.split(";")[0].strip()
            if line and not line.startswith("."):
                body.append(line)
            elif line.endswith(":"):
                body.append(line)
        out.setdefault(m.group(1), body)
    return out


def loops(body):
    """(first line, last line) of every backward branch's span"""
    where = {l[:-1]: i for i, l in enumerate(body) if l.endswith(":")}
    for i, l in enumerate(body):
        m = re.match(r"s_cbranch_\w+\s+(\S+)|s_branch\s+(\S+)", l)
        if m and (m.group(1) or m.group(2)) in where and where[m.group(1) or m.group(2)] < i:
            yield where[m.group(1) or m.group(2)], i


def vm_waits(lines):
    c = collections.Counter()
    for l in lines:
        m = re.match(r"s_waitcnt.*vmcnt\((\d+)\)", l)
        if m:
            c[int(m.group(1))] += 1
    return dict(sorted(c.items()))


if sys.argv[1] == "waits":
    ks = kernels(sys.argv[2])
    for frag in sys.argv[3:]:
        for name, body in ks.items():
            if frag not in name:
                continue
            a, b = max(loops(body), key=lambda ab: ab[1] - ab[0], default=(0, 0))
            print(name)
            print("    walk loop: %d lines, vmcnt(N) by N: %s" % (b - a, vm_waits(body[a:b])))
            print("    whole kernel: vmcnt(N) by N: %s" % vm_waits(body))
else:
    ka, kb = kernels(sys.argv[2]), kernels(sys.argv[3])
    strip = lambda body: [l for l in body if not l.endswith(":")]
    for name in sorted(set(ka) | set(kb)):
        if name not in ka or name not in kb:
            print("ONLY IN ONE ", name)
        elif strip(ka[name]) == strip(kb[name]):
            print("same        ", name)
        else:
            print("DIFFERENT   ", name)
