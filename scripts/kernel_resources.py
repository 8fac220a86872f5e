"""Register / scratch / occupancy of every step kernel of the given specs.inc entries and generic
register-row lengths, from the compiler's own accounting (hipcc -Rpass-analysis=kernel-resource-usage
on spec.hip / generic.hip; same flags as csrc/Makefile).
usage: kernel_resources.py <spec id | generic:NR> ... > profiles/<round>_kernel_resources.txt
       kernel_resources.py all    (every specs.inc entry, then every GENERIC_NRS of the Makefile)"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mjlab-1_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function",
         "-fno-hip-fp32-correctly-rounded-divide-sqrt", "-DMJX_HDR_HASH=0x1ULL"]
names = {}
for line in open(os.path.join(CSRC, "specs.inc")):
  m = re.match(r"MJX_SPEC\((\d+), (\w+),.*, (\d+), (\d+)\)$", line.strip())
  if m:
    names[m.group(1)] = f"{m.group(2)} {m.group(3)}/{m.group(4)}"


def resources(target):
  """(label, {mangled kernel: {v, a, s, o}}) of one spec id or generic:NR"""
  if target.startswith("generic:"):
    define, src, label = f"-DMJX_GENERIC_NR={target[8:]}", "generic.hip", target
  else:
    define, src, label = f"-DMJX_SPEC_ID={target}", "spec.hip", target + " " + names.get(target, "")
  with tempfile.TemporaryDirectory() as tmp:
    r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, define, "-c", "-o",
                        os.path.join(tmp, "s.o"), src, "-Rpass-analysis=kernel-resource-usage"],
                       cwd=CSRC, capture_output=True, text=True)
  if r.returncode != 0:
    raise SystemExit(f"kernel_resources: {label}: hipcc failed\n{r.stderr[-2000:]}")
  cur, rows = None, {}
  for line in r.stderr.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
      cur = m.group(1)
      rows[cur] = {}
      continue
    for key, pat in (("v", r"VGPRs: (\d+)"), ("a", r"AGPRs: (\d+)"), ("s", r"ScratchSize \[bytes/lane\]: (\d+)"),
                     ("o", r"Occupancy \[waves/SIMD\]: (\d+)")):
      m = re.search(pat, line)
      if m and cur:
        rows[cur][key] = m.group(1)
  return label, rows


targets = sys.argv[1:]
if targets == ["all"]:
  nrs = re.search(r"^GENERIC_NRS = (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
  targets = list(names) + [f"generic:{nr}" for nr in nrs.split()]
print(f"{'spec':28s} {'kernel':34s} {'VGPR':>5s} {'AGPR':>5s} {'scratch B/lane':>14s} {'waves/SIMD':>10s}")
with ThreadPoolExecutor(int(os.environ.get("MAX_JOBS", min(16, os.cpu_count() or 1)))) as pool:
  for label, rows in pool.map(resources, targets):
    for k, v in rows.items():
      dm = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
      dm = dm.replace("mjx::", "").split("(")[0]
      print(f"{label:28s} {dm:34s} {v.get('v', '-'):>5s} {v.get('a', '-'):>5s} "
            f"{v.get('s', '-'):>14s} {v.get('o', '-'):>10s}", flush=True)
