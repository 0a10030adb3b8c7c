"""Recipe for oracle/_ref/: the reference's OWN AudioSDR.cpp, AudioIQgenerator.cpp, AudioGrabberComplex256.cpp and AudioSDRpreProcessor.cpp,
compiled by path from the reference tree against the stand-in Teensy / CMSIS headers of oracle/ref_shim/ (README there), and the helpers
that run the two binaries.  Nothing of the reference is copied into the repository: the binaries and their manifest live in oracle/_ref/,
which git ignores.  TEST INFRASTRUCTURE ONLY.

    build()   compiles ref_driver and ref_front_driver when the reference tree is present and oracle/_ref/ is missing or was built from
              other stand-in, driver or reference files or other flags (MANIFEST.json); without the tree it leaves oracle/_ref/ alone.
    status()  ("ok" | "missing" | "stale", detail): the binaries are there, and the manifest's stand-in and driver hashes and flags equal
              oracle/ref_shim/ and FLAGS as they are now.  The tests fail on "stale": an edited stand-in is not trusted until rebuilt.
"""
import hashlib
import json
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHIM = os.path.join(HERE, "ref_shim")
OUT = os.path.join(HERE, "_ref")
MANIFEST = os.path.join(OUT, "MANIFEST.json")
REF_TREE = os.environ.get("ASDR_REFERENCE_TREE", "/root/reference")
REF_SRC = os.path.join(REF_TREE, "SRC", "AudioSDRlib")
CXX = os.environ.get("CXX", "g++")
# -ffp-contract=off: every float operation separately rounded, as on the reference's target; static C++ runtime: the binaries run on
# machines without this toolchain
FLAGS = ["-std=gnu++14", "-fpermissive", "-w", "-O2", "-ffp-contract=off", "-static-libstdc++", "-static-libgcc"]
# binary -> (driver in oracle/ref_shim/, reference sources compiled by path)
TARGETS = {
    "ref_driver": ("ref_driver.cpp", ["AudioSDR.cpp"]),
    "ref_front_driver": ("ref_front_driver.cpp", ["AudioIQgenerator.cpp", "AudioGrabberComplex256.cpp", "AudioSDRpreProcessor.cpp"]),
}
EXE = {name: os.path.join(OUT, name) for name in TARGETS}


def _sha256(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def _code_files(top):
    out = {}
    for d, _, files in os.walk(top):
        for n in files:
            if n.endswith((".h", ".cpp")):
                p = os.path.join(d, n)
                out[os.path.relpath(p, top)] = _sha256(p)
    return dict(sorted(out.items()))


def shim_hashes():
    """sha256 of every stand-in header and driver under oracle/ref_shim/ (the README is documentation, not code)."""
    return _code_files(SHIM)


def reference_tree_present():
    return all(os.access(os.path.join(REF_SRC, s), os.R_OK) for _, srcs in TARGETS.values() for s in srcs)


def read_manifest():
    try:
        with open(MANIFEST) as f:
            return json.load(f)
    except (OSError, ValueError):
        return None


def status():
    """("ok" | "missing" | "stale", detail) of oracle/_ref/ against the stand-ins, drivers and flags as they are now."""
    m = read_manifest()
    missing = [os.path.relpath(p, HERE) for p in list(EXE.values()) + [MANIFEST] if not os.path.exists(p)]
    if missing or m is None:
        return "missing", "oracle/_ref/ is not built (%s)" % ", ".join(missing or ["unreadable MANIFEST.json"])
    now, then = shim_hashes(), m.get("shim_sha256", {})
    if now != then:
        diff = sorted(n for n in set(now) | set(then) if now.get(n) != then.get(n))
        return "stale", "oracle/ref_shim/ differs from what oracle/_ref/ was built from: %s" % ", ".join(diff)
    if m.get("flags") != FLAGS:
        return "stale", "oracle/_ref/ was built with %s, the recipe says %s" % (m.get("flags"), FLAGS)
    return "ok", "built from %d stand-in / driver files and %d reference sources" % (len(then), len(m.get("reference_sha256", {})))


def build(force=False, log=print):
    """Compile oracle/_ref/ref_driver and ref_front_driver and write MANIFEST.json (sha256 of every reference source compiled, of every
    stand-in and driver, and the flags).  Returns status()."""
    if not reference_tree_present():
        if os.path.isdir(OUT):
            log("oracle/_ref: no reference tree at %s; the existing oracle/_ref/ is left as it is (%s)" % (REF_TREE, status()[1]))
        else:
            log("oracle/_ref: no reference tree at %s and no oracle/_ref/; nothing to build" % REF_TREE)
        return status()
    want = {"flags": FLAGS, "shim_sha256": shim_hashes(), "reference_sha256": _code_files(REF_SRC),     # (.cpp and the headers they include)
            "targets": {n: {"driver": d, "reference_sources": s} for n, (d, s) in TARGETS.items()}}
    have = read_manifest()
    if not force and have == want and all(os.path.exists(p) for p in EXE.values()):
        return status()
    os.makedirs(OUT, exist_ok=True)
    if os.path.exists(MANIFEST):
        os.remove(MANIFEST)                       # a failed build must not leave a manifest that vouches for older binaries
    for name, (driver, srcs) in TARGETS.items():
        tmp = EXE[name] + ".tmp"
        subprocess.check_call([CXX] + FLAGS + ["-I", SHIM, "-I", REF_SRC, os.path.join(SHIM, driver)] +
                              [os.path.join(REF_SRC, s) for s in srcs] + ["-o", tmp])
        os.replace(tmp, EXE[name])
    with open(MANIFEST, "w") as f:
        json.dump(want, f, indent=1, sort_keys=True)
    log("oracle/_ref: built %s" % ", ".join(sorted(TARGETS)))
    return status()


# ---------------------------------------------------------------------------------------------------------------------------------------
# Running the binaries: one fresh child process per reference instance (the reference keeps function-statics: one instance per process).
INT_GETTERS = ["getDemodMode", "getMute", "getAudioFilter", "ALSfilterIsEnabled", "ALSfilterIsNotch", "ALSfilterIsPeak", "ALSfilterIsAdaptive",
               "AGCisEnabled", "AGCisActive", "NoiseBlankerisEnabled", "NoiseBlankerDetection", "getSAMphaseLockStatus"]
F32_GETTERS = ["getTuningOffset", "getBPFlower", "getBPFupper", "getAGCthreshold", "getAGCslope", "getAGCkneeWidth", "getAGCattack", "getAGCrelease",
               "getAAGalphaAttack", "getAGCbetaAttack", "getAGCalphaRelease", "getAGCbetaRelease", "getAGCstaticGain", "getAMcarrierLevel", "getSAMfrequency"]


def _run(args, tmp):
    p = subprocess.run(args, capture_output=True, text=True, timeout=300, cwd=tmp)
    if p.returncode != 0:
        raise RuntimeError("%s %s exited %d: %s" % (os.path.basename(args[0]), args[1], p.returncode, p.stderr.strip()))
    return p.stdout


def _iq_file(tmp, I, Q):
    path = os.path.join(tmp, "iq.bin")
    np.stack([np.asarray(I, np.int16).reshape(-1, 128), np.asarray(Q, np.int16).reshape(-1, 128)], axis=1).tofile(path)   # [blocks][2][128]
    return path


def run_sdr(script, I, Q):
    """The reference's AudioSDR on one channel.  script: (method, args) pairs; ("run", (k,)) feeds the next k blocks (setters between
    blocks), what is left is fed at the end.  I, Q: int16 [blocks][128].  Returns (audio int16 [blocks][128], getters): getters maps the
    integer getters to ints, the float ones to their float32 bit patterns and "getAGClookup" to the 129 bit patterns of the table."""
    nb = np.asarray(I).reshape(-1, 128).shape[0]
    with tempfile.TemporaryDirectory() as tmp:
        sp, out = os.path.join(tmp, "script.txt"), os.path.join(tmp, "out.bin")
        with open(sp, "w") as f:
            f.write("".join(" ".join([m] + [repr(float(a)) for a in args]) + "\n" for m, args in script))
        text = _run([EXE["ref_driver"], sp, _iq_file(tmp, I, Q), str(nb), out], tmp)
        audio = np.fromfile(out, dtype=np.int16).reshape(nb, 128)
    g = {}
    for line in text.splitlines():
        k, *v = line.split()
        g[k] = [int(x, 16) for x in v] if k == "getAGClookup" else int(v[0], 16) if k in F32_GETTERS else int(v[0])
    assert set(g) == set(INT_GETTERS) | set(F32_GETTERS) | {"getAGClookup"} and len(g["getAGClookup"]) == 129, sorted(g)
    return audio, g


def run_iqgen(balance, x):
    """AudioIQgenerator (balance 0.0: setGainBalance never called).  x: int16 [blocks][128] -> (I, Q) int16 [blocks][128]."""
    x = np.asarray(x, np.int16).reshape(-1, 128)
    with tempfile.TemporaryDirectory() as tmp:
        xf, of = os.path.join(tmp, "x.bin"), os.path.join(tmp, "o.bin")
        x.tofile(xf)
        _run([EXE["ref_front_driver"], "iqgen", repr(float(balance)), xf, str(x.shape[0]), of], tmp)
        r = np.fromfile(of, dtype=np.int16).reshape(-1, 2, 128)
    return r[:, 0].copy(), r[:, 1].copy()


def run_grab(I, Q, after):
    """AudioGrabberComplex256 fed I, Q int16 [blocks][128], grab() after block `after`.  Returns (buffer int16 [512],
    newDataAvailable() before the grab, after it)."""
    nb = np.asarray(I).reshape(-1, 128).shape[0]
    with tempfile.TemporaryDirectory() as tmp:
        of = os.path.join(tmp, "g.bin")
        text = _run([EXE["ref_front_driver"], "grab", _iq_file(tmp, I, Q), str(nb), str(after), of], tmp)
        buf = np.fromfile(of, dtype=np.int16)
    flags = [int(l.split()[1]) for l in text.splitlines()]
    return buf, flags[0], flags[1]


def run_pre_fixed(correction, swap, I, Q):
    """AudioSDRpreProcessor with the detector stopped and a fixed correction and swap.  Returns (I, Q int16 [blocks][128],
    getI2SerrorCompensation(), getAutoI2SerrorDetectionStatus())."""
    nb = np.asarray(I).reshape(-1, 128).shape[0]
    with tempfile.TemporaryDirectory() as tmp:
        of = os.path.join(tmp, "p.bin")
        text = _run([EXE["ref_front_driver"], "pre", str(int(correction)), str(int(swap)), _iq_file(tmp, I, Q), str(nb), of], tmp)
        r = np.fromfile(of, dtype=np.int16).reshape(nb, 2, 128)
    g = {l.split()[0]: int(l.split()[1]) for l in text.splitlines()}
    return r[:, 0].copy(), r[:, 1].copy(), g["getI2SerrorCompensation"], g["getAutoI2SerrorDetectionStatus"]


def _per_block(text, of, nb):
    r = np.fromfile(of, dtype=np.int16).reshape(nb, 2, 128)
    rows = [[int(v) for v in l.split()] for l in text.splitlines()]
    assert [x[0] for x in rows] == list(range(nb)) and all(len(x) == 3 for x in rows), text[:200]
    return r[:, 0].copy(), r[:, 1].copy(), np.array([x[1] for x in rows]), np.array([x[2] for x in rows])


def run_pre_auto(I, Q, correction=0, swap=0, n_fixed=0, restarts=()):
    """AudioSDRpreProcessor: setI2SerrorCompensation(correction) and swapIQ(swap), n_fixed blocks with that correction, then
    startAutoI2SerrorDetection(), and again before every block in `restarts`.  Returns (I, Q int16 [blocks][128], and after every
    block getI2SerrorCompensation() and getAutoI2SerrorDetectionStatus())."""
    nb = np.asarray(I).reshape(-1, 128).shape[0]
    with tempfile.TemporaryDirectory() as tmp:
        of = os.path.join(tmp, "p.bin")
        text = _run([EXE["ref_front_driver"], "pre-auto", str(int(correction)), str(int(swap)), str(int(n_fixed)),
                     ",".join(str(int(b)) for b in restarts) or "-", _iq_file(tmp, I, Q), str(nb), of], tmp)
        return _per_block(text, of, nb)


def run_pre_script(script, I, Q):
    """AudioSDRpreProcessor with setters between blocks: script of (method, args) pairs -- startAutoI2SerrorDetection,
    stopAutoI2SerrorDetection, setI2SerrorCompensation (c,), swapIQ (s,), run (k,).  Returns what run_pre_auto returns."""
    nb = np.asarray(I).reshape(-1, 128).shape[0]
    with tempfile.TemporaryDirectory() as tmp:
        sp, of = os.path.join(tmp, "script.txt"), os.path.join(tmp, "p.bin")
        with open(sp, "w") as f:
            f.write("".join(" ".join([m] + [str(int(a)) for a in args]) + "\n" for m, args in script))
        text = _run([EXE["ref_front_driver"], "pre-script", sp, _iq_file(tmp, I, Q), str(nb), of], tmp)
        return _per_block(text, of, nb)


if __name__ == "__main__":
    print(build())
