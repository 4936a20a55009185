"""Compare two hipcc -S device assembly files function by function.

usage: asmdiff.py OLD.s NEW.s [-v]
Local labels are renumbered in order of appearance and comments dropped, so that a function whose
instructions are the same compares equal wherever it lies in the file.  Prints the functions whose
instruction streams differ with their old and new instruction counts (-v: a unified diff as well).
"""
import difflib
import re
import sys


def functions(path):
    out, name, body = {}, None, []
    for line in open(path):
        line = line.split(";")[0].rstrip()
        if name is None:
            m = re.match(r"^([A-Za-z_][\w$.]*):\s*$", line)
            if m and not m.group(1).startswith(".L"):
                name, body = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
        elif line.strip() and not line.lstrip().startswith((".p2align", ".loc", ".cfi", ".file")):
            body.append(line.strip())
    return out


def normal(body):
    ids = {}
    return [re.sub(r"\.L[A-Za-z_]*\d+(_\d+)?", lambda m: ids.setdefault(m.group(0), ".L%d" % len(ids)), l) for l in body]


def count(body):
    return sum(1 for l in body if not l.endswith(":") and not l.startswith("."))


old, new = functions(sys.argv[1]), functions(sys.argv[2])
for f in sorted(set(old) | set(new)):
    a, b = normal(old.get(f, [])), normal(new.get(f, []))
    if a != b:
        print(f"{f}: {count(a) if f in old else 'absent'} -> {count(b) if f in new else 'absent'} instructions")
        if "-v" in sys.argv:
            print("\n".join(difflib.unified_diff(a, b, "old", "new", lineterm="", n=2)))
print(f"{len(old)} functions before, {len(new)} after")
