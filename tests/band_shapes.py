"""What the band tests share (tests/test_band_host.py, tests/test_gpu_factored_band.py): the shapes K-factored's
planner makes of a grid -- q-tiles with one q (covest_amd/csrc/plan_factored.cpp shared_order), key tiles
(tiles_host.cpp cut_tiles) -- restated in Python, covest_amd/csrc/band.h run on them through tests/band_check.cpp, and
the exact weighted terms of covest/models.py:211-242 in the log domain to judge a band by."""
import math
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "covest_amd", "csrc")
STEP = 4          # copy numbers of an MFMA step
TILE = 32         # keys of a key tile
GAP_FILL = 12     # host.h kGapFill: gaps of up to this many keys are bridged with filler keys
MIN_SHARED = 3    # tiles.h kMinSharedSteps
CHUNK = 512       # copy numbers of one workgroup: longer weight vectors go chunk by chunk, without shared steps
S = 8             # error classes of a plain grid
MIN_BAND = 8      # band.h kBandMinShared: a unit with fewer shared steps has no band


def host_compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        exe = shutil.which(name) if name else None
        if exe:
            return exe
    return None


def build_band_check(out_dir, sanitize=False):
    cxx = host_compiler()
    assert cxx is not None, "no host C++ compiler: the band's proof cannot be checked"
    exe = os.path.join(str(out_dir), "band_check_san" if sanitize else "band_check")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    build = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror"] + flags +
                           ["-I", CSRC, os.path.join(HERE, "band_check.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=120)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def run_band_check(exe, cases):
    """cases: rows of (rate0, ln_rate[8], ln_comb[8], ln(1-q), o_ref_max, n_steps, key_first, key_last) -> (step_lo, step_hi)
    per row (step_lo = 1 + 4 trips of 16 copy numbers cut at the lower edge, 0: none)."""
    text = "".join(" ".join(repr(float(v)) for v in row) + "\n" for row in cases)
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    out = [tuple(int(x) for x in line.split()) for line in run.stdout.splitlines()]
    assert len(out) == len(cases) and all(lo == 0 or (lo % 4 == 1 and 1 < lo < hi) for lo, hi in out), out[:8]
    return out


def classes(k, r, c, e):
    """The error classes' rates and weights: covest/models.py:71-79, :25."""
    ck = c * (r - k + 1) / r
    rates = np.array([ck * 3.0 ** -s * (1.0 - e) ** (k - s) * e ** s for s in range(S)])
    comb = np.array([float(math.comb(k, s)) * 3.0 ** s for s in range(S)])
    return rates, comb


def threshold_o(q1, q2, q, hist_size, threshold=1e-8):
    """covest/models.py:185-208."""
    def b_o(o):
        return q1 if o == 1 else (1 - q1) * q2 if o == 2 else (1 - q1) * (1 - q2) * q * (1 - q) ** (o - 3)
    for o in range(1, hist_size):
        if b_o(o) <= threshold:
            return o
    return hist_size


def q_tiles(q1s, q2s, qs, hist_size):
    """The q-tiles of a grid whose tiles have one q each: {q, t_lo, t_hi, nsh, n_steps} (nsh = 0: no shared steps,
    the unit has no band)."""
    tiles = []
    for q in qs:
        ts = sorted((threshold_o(q1, q2, q, hist_size) for q1 in q1s for q2 in q2s), reverse=True)
        for at in range(0, len(ts), 16):
            grp = ts[at:at + 16]
            t_hi, t_lo = grp[0], grp[-1]
            n = (t_lo - (STEP + 1)) // STEP
            tiles.append({"q": float(q), "t_lo": t_lo, "t_hi": t_hi, "n_steps": (t_hi - 1 + STEP - 1) // STEP,
                          "nsh": n if (t_hi - 1 <= CHUNK and n >= MIN_SHARED) else 0})
    return tiles


def key_tiles(keys):
    """(first key, keys) of every key tile."""
    keys = sorted(keys)
    tiles, i = [], 0
    while i < len(keys):
        j = i + 1
        while j < len(keys) and keys[j] - keys[j - 1] <= GAP_FILL + 1:
            j += 1
        for k0 in range(keys[i], keys[j - 1] + 1, TILE):
            tiles.append((k0, min(TILE, keys[j - 1] - k0 + 1)))
        i = j
    return tiles


def band_case(rates, comb, qt, k0):
    """The arguments the kernel hands band.h for a unit of q-tile `qt` in the key tile that starts at k0 (the rows past a
    short tile's keys counted in, as the kernel does)."""
    with np.errstate(divide="ignore"):
        ln_rate, ln_comb = np.log(rates), np.log(comb)
    return [rates[0]] + list(ln_rate) + list(ln_comb) + [math.log1p(-qt["q"]), 4 + 4 * qt["nsh"], qt["n_steps"], k0, k0 + TILE - 1]


def log_terms(rates, comb, o_top, keys):
    """lg[o - 1, j] = ln sum_s comb_s e^(-o l_s) (o l_s)^j / N(o), without the 1 / j! every term of a key shares:
    a_os TP(o l_s, j) of covest/models.py:220-240 with the (1 - e^(-o l_s)) of numerator and denominator cancelled."""
    o = np.arange(1, o_top + 1, dtype=np.float64)[:, None, None]
    j = np.asarray(keys, dtype=np.float64)[None, :, None]
    live = (rates > 0) & (comb > 0)
    lam, cb = rates[live][None, None, :], comb[live][None, None, :]
    n_o = np.sum(cb * -np.expm1(-o * lam), axis=2)          # [o, 1]
    t = np.log(cb) - o * lam + j * np.log(o * lam)            # [o, j, s]
    top = t.max(axis=2)
    return top + np.log(np.sum(np.exp(t - top[:, :, None]), axis=2)) - np.log(n_o)


def outside_share(lg, qt, band):
    """The largest share, over the keys of lg's columns, of the weighted terms outside band = (step_lo, step_hi) -- the
    steps 1 .. step_lo - 1 and those from step_hi on -- in a column's sum: an upper bound of it that holds for every
    column of the q-tile, the dropped copy numbers up to the LARGEST cut-off against the geometric terms (o >= 3) below
    the SMALLEST one."""
    step_lo, step_hi = band
    ln_r = math.log1p(-qt["q"])
    o = np.arange(1, lg.shape[0] + 1, dtype=np.float64)[:, None]
    w = lg + (o - 3.0) * ln_r
    w = w - w[2:qt["t_lo"] - 1].max(axis=0)
    kept = np.exp(w[2:qt["t_lo"] - 1]).sum(axis=0)
    dropped = np.exp(w[STEP * step_hi:qt["t_hi"] - 1]).sum(axis=0) + np.exp(w[STEP:STEP * max(step_lo, 1)]).sum(axis=0)
    return float((dropped / kept).max())
