"""What the bordered pyramid export buys a drop-in host, measured on a GPU box from the repo root:
  - the per-call latency of the drop-in ORBextractor facade (tests/cpp/facade_latency.cpp, one 752 x 480 image per call, 300 calls, like
    tools/gpu_facade_latency.sh) with mvImagePyramid exported and without;
  - stereo pairs per second of the reference's unchanged stereo Frame constructor on the drop-in (ref_frame_stereo_repeat in
    oracle/_ref/libref_frame_dropin.so, one pair of long-lived extractors), and of the all-reference build (libref_frame.so) beside it.
--lib-dir / --include / --dropin point at another build (the parent commit's library, facade header and drop-in Frame library) for the "before" rows.
Writes one JSON file (default profiles/dropin_export/<label>.json) and prints it.
    python tools/bench_dropin_frame.py --label after
    python tools/bench_dropin_frame.py --label before --lib-dir B --include B/include/orb_slam3_amd --dropin B/libref_frame_dropin.so"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="after")
    ap.add_argument("--lib-dir", default=os.path.join(ROOT, "orb_slam3_detailed_comments_amd"))
    ap.add_argument("--include", default=os.path.join(ROOT, "include", "orb_slam3_amd"))
    ap.add_argument("--dropin", default=os.path.join(ROOT, "oracle", "_ref", "libref_frame_dropin.so"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from orb_slam3_detailed_comments_amd import synth
    import oracle_lib as ol
    tmp = tempfile.mkdtemp(prefix="dropin_bench_")
    ims = {"stereo_left": synth.stereo_pair(752, 480, seed=100)[0], "natural": synth.natural(752, 480, seed=100)}
    exe = os.path.join(tmp, "facade_latency")
    subprocess.run(["g++", "-std=c++14", "-O2", "-w", "-DORBX_FACADE", "-I" + a.include, "-I" + os.path.join(ROOT, "oracle", "opencv_shim"),
                    os.path.join(ROOT, "tests", "cpp", "facade_latency.cpp"), "-L" + a.lib_dir, "-lorbx_hip", "-Wl,-rpath," + os.path.abspath(a.lib_dir),
                    "-o", exe], check=True)
    res = {"label": a.label, "lib_dir": os.path.relpath(os.path.abspath(a.lib_dir), ROOT), "facade_ms_per_call": {}}
    for name, im in ims.items():
        raw = os.path.join(tmp, name + ".raw"); im.tofile(raw)
        row = {}
        for exp in (1, 0):
            out = subprocess.run(["timeout", "-k", "10", "300", exe, raw, "752", "480", "1200", str(a.calls), str(exp)], capture_output=True, text=True, check=True).stdout
            row["export_on" if exp else "export_off"] = float(re.search(r"([0-9.]+) ms per call", out).group(1))
            print(out.strip(), flush=True)
        res["facade_ms_per_call"][name] = row
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]))
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tests", "dropin_repeat_runner.py"), os.path.join(a.lib_dir, "liborbx_hip.so"),
                        "752", "480", "100", str(a.seconds), a.dropin], capture_output=True, text=True, env=env, check=True)
    res["dropin_frame"] = json.loads(r.stdout.strip().splitlines()[-1])
    n, el, m, orb_ms, st_ms = ol.reference_frame_repeat(*synth.stereo_pair(752, 480, seed=100), a.seconds)
    res["reference_frame"] = {"frames": n, "seconds": el, "matches": m, "pairs_per_s": n / el, "orb_ms_per_pair": orb_ms / n, "stereo_ms_per_pair": st_ms / n}
    out = a.out or os.path.join(ROOT, "profiles", "dropin_export", a.label + ".json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
