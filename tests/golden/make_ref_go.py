#!/usr/bin/env python3
"""Regenerate tests/golden/ref_go.json.

What tests/test_abi.py needs to know about the reference's Go tree, kept as
DATA so that the tests run without the tree:

  "names"        the top-level identifiers (functions, types, variables,
                 constants) of the non-test files of each package directory
                 the shim and the caller files are added to;
  "header_all"   package header's identifiers with its method names too (the
                 wider set test_go_shim_names_do_not_collide... compares);
  "patch_hunks"  for every hunk of go/netstack-hipcsum.patch: the file, the
                 hunk's old start line and length, the line of the reference's
                 file at which those old lines are found (`applies_at`; equal
                 to the start when the hunk applies without an offset), and
                 the SHA-256 of the reference's lines there.  The test hashes
                 the patch's own old side (context and removed lines) and
                 compares: equal digests mean the hunk applies exactly.

Nothing here is reference source: the file holds names, line numbers and
digests only.

  python tests/golden/make_ref_go.py REFERENCE_ROOT   (the directory holding tcpip/)
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PATCH = os.path.join(ROOT, "go", "netstack-hipcsum.patch")
PACKAGES = ("tcpip/header", "tcpip/transport/tcp", "tcpip/link/fdbased")


def go_code(src):
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    return re.sub(r'"(?:[^"\\\n]|\\.)*"|`[^`]*`', '""', src)


def top_level(code, methods=False):
    fn = r"^func (?:\([^)]*\)\s*)?(\w+)\(" if methods else r"^func (\w+)\("
    names = set(re.findall(fn, code, flags=re.M)) | set(re.findall(r"^type (\w+)\b", code, flags=re.M))
    names |= set(re.findall(r"^(?:var|const)\s+(\w+)", code, flags=re.M))
    for blk in re.findall(r"^(?:const|var) \((.*?)^\)", code, flags=re.M | re.S):
        names |= set(re.findall(r"^\s*(\w+)", blk, flags=re.M))
    return names


def package_names(d, methods=False):
    out = set()
    for fn in sorted(os.listdir(d)):
        if fn.endswith(".go") and not fn.endswith("_test.go"):
            out |= top_level(go_code(open(os.path.join(d, fn)).read()), methods)
    return sorted(out)


def patch_hunks(text):
    """[(file, old_start, [old lines])] of a unified diff."""
    hunks, cur, name = [], None, None
    for line in text.split("\n"):
        if line.startswith("--- "):
            cur = None
        elif line.startswith("+++ b/"):
            name = line[6:].strip()
        elif line.startswith("@@"):
            start = int(re.match(r"@@ -(\d+)", line).group(1))
            cur = (name, start, [])
            hunks.append(cur)
        elif cur is not None and line[:1] in (" ", "-"):
            cur[2].append(line[1:])
    return hunks


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def main():
    ref = sys.argv[1]
    out = {"names": {p: package_names(os.path.join(ref, p)) for p in PACKAGES},
           "header_all": package_names(os.path.join(ref, "tcpip/header"), methods=True),
           "patch_hunks": []}
    for name, start, old in patch_hunks(open(PATCH).read()):
        lines = open(os.path.join(ref, name)).read().split("\n")
        at = [k + 1 for k in range(len(lines) - len(old) + 1) if lines[k:k + len(old)] == old]
        at.sort(key=lambda k: abs(k - start))
        if not at:
            raise SystemExit(f"{name} @@ -{start}: the hunk's old lines are not in the reference")
        k = at[0]
        out["patch_hunks"].append({"file": name, "old_start": start, "old_lines": len(old), "applies_at": k,
                                   "sha256": digest(lines[k - 1:k - 1 + len(old)])})
    with open(os.path.join(HERE, "ref_go.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
