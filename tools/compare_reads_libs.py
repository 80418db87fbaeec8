"""Two builds of the library side by side on the file front end (covest_reads_open / _next / _bytes, csrc/reads_io.cpp):
what a change did to the batches, and to the time of reading.  Host code only; no device is needed.

For each library, in a child process of its own (COVEST_AMD_LIB is read at import): a generated corpus -- the small
shapes of tests/reads_parse_check.cpp written to files, 3000 ragged FASTA reads, and a FASTQ of more than 3 MiB whose
lines start to wrap behind the first 2 MiB (the 4-line parser then works in several pieces when it has to hand over, and
the first look at the file has said "not wrapped") -- streamed through ReadBatches._next with batches of 1, 1000, 2^22
and 2^26 bases, COVEST_READER_THREADS 1, 3 and 16, and the three N strategies.  One line per run: the number of batches,
reads and bases, covest_reads_bytes at the end, and a SHA-256 over every batch's (n_reads, n_bases, covest_reads_bytes
after it, bases, offsets); a failure adds the exception ReadBatches makes of it, return code and whole message.
Required: the two outputs are the same file.  They stay in the work directory; --out keeps a digest: per file of the
corpus the runs, the failures among them, a SHA-256 over its run lines and each distinct failure message.

    python tools/compare_reads_libs.py --new covest_amd/lib/libcovest_amd.so --parent /path/lib_parent.so \\
        [--work DIR] [--out profiles/reads_refactor_cmp.txt]
    python tools/compare_reads_libs.py --time --new ... --parent ... [--out profiles/reads_refactor_ab.txt]

--time: wall time of reading, without counting, a generated FASTA and a generated FASTQ of about 1 Gbase of 150-base
reads each, default thread count; one discarded pass per file warms the page cache, then the libraries alternate over
five rounds, each pass in a fresh process.  Accepted when the new median is at most the parent's median * (1 + s),
s = (parent's max - min) / parent's median of the same session.
"""
import argparse
import ctypes
import hashlib
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BATCHES = (1, 1000, 1 << 22, 1 << 26)
THREADS = (1, 3, 16)
PLAIN = "".join("@p%d\nACGTACGTAC\n+\nIIIIIIIIII\n" % i for i in range(400))


def small_shapes():
    """(file name, text) of the shapes at which the parser can go wrong (tests/reads_parse_check.cpp has the same)."""
    out = [("empty.fa", ""), ("header_only.fa", ">h"), ("header_line.fa", ">h\n"), ("no_trailing_newline.fa", ">a\nACGT\n>b\nGG"),
           ("crlf.fa", ">a\r\nACGT\r\nAC\r\n>b\r\nGn\r\n"),
           ("text_first.fa", "text before the first header\nACGT\n>r1 some description\nACGTNACGTACG\r\nTTTGACA\n>empty\n>r2\nNNACGTACGTAC"),
           ("empty_records.fa", ">a\n>b\n>c\nAC\n\n>d\n"), ("no_header.fa", "no header anywhere\nACGT\n"),
           ("bad_base.fa", ">x\nACGT\nACRT\n"),
           ("empty.fq", ""), ("header_only.fq", "@h"), ("ends_in_sequence.fq", "@r\nACGT"),
           ("blank_lines.fq", "@a\nACGT\n+\nIIII\n\n\n@b\nTTGN\n+\n@III\n\r\n@c\nGG\n+\n+I\n@d\nAC\n+\nII\n\n\n\n"),
           ("crlf.fq", "@a\r\nACGT\r\n+\r\nIIII\r\n\r\n@b\r\nGG\r\n+\r\nII\r\n"),
           ("wrapped_sequence.fq", "@a\nACNN\nNGT\n+\nIIII\nIII\n\n@b\nAC\n+\n@I\n"),
           ("wrapped_quality.fq", "@a\nACGTACGT\n+\nIIII\n@III\n@x\nTTTTGGGG\n+\nIIIIIIII\n"),
           ("quality_wraps_late.fq", PLAIN + "@w\nACGTACGT\n+\nIIII\n@III\n@x\nTTTTGGGG\n+\nIIIIIIII\n"),
           ("quality_wraps_late_and_short.fq", PLAIN + "@w\nACGTACGT\n+\nIIII\n@III\n@x\nTTTTGGGG\n+\nIII\n"),
           ("sequence_wraps_late.fq", PLAIN + "@w\nACGT\nACGT\n+\nIIIIIIII\n@y\nGG\n+\nII\n"),
           ("ends_in_wrapped_sequence.fq", "@a\nACGT\nAC\n+\nIIIIII\n@b\nAC\nGT"), ("ends_in_quality.fq", "@a\nACGT\nACGT\n+\nIIIIII\n"),
           ("quality_too_long.fq", "@a\nACGT\n+\nIIII\nII\n@b\nAC\n+\nII\n"), ("first_line_without_at.fq", "ACGT\n+\nIIII\n"),
           ("third_line_without_plus.fq", "@a\nACGT\n\nIIII\n"), ("bad_base_strict.fq", "@x\nACGU\n+\nIIII\n"),
           ("bad_base_general.fq", "@a\nACGT\nAXGT\n+\nIIIIIIII\n")]
    rng = random.Random(7)
    lines = []
    for n in (15, 16, 17, 31, 32, 33):  # the 16-byte block of put_line and its remainder
        lines.append(">clean\n%s\n" % ("G" * n))
        for place in sorted({0, 15, n - 1}):
            if place >= n:
                continue
            for c in "Nn X":
                line = [rng.choice("ACGTacgt") for _ in range(n)]
                line[place] = c
                if c == "X":
                    out.append(("bad_letter_%d_%d.fa" % (n, place), ">ok\nAC\n>r\n" + "".join(line)))
                else:
                    lines.append(">r\n%s\n" % "".join(line))
    out.append(("line_lengths.fa", "".join(lines)))
    return out


def large_shapes():
    rng = random.Random(5)
    fa = []
    for i in range(3000):  # as tests/test_reads_io.py
        r = "".join(rng.choice("ACGTNacgtn") for _ in range(rng.randint(0, 400)))
        fa.append(">read_%d %s\n" % (i, "x" * rng.randint(0, 50)))
        fa += [r[j:j + 70] + "\n" for j in range(0, len(r), 70)]
    fq, size, i = [], 0, 0
    while size < (7 << 19):  # 3.5 MiB: 4-line records for 2 MiB, then sequences and qualities over lines of 60
        seq = "".join(rng.choice("ACGTN" if i % 40 == 0 else "ACGT") for _ in range(rng.randint(1, 300)))
        qual = ("@" if i % 3 else "+") + "I" * (len(seq) - 1)
        width = 60 if size >= (2 << 20) else len(seq)
        rec = "@r%d\n%s+\n%s" % (i, "".join(seq[j:j + width] + "\n" for j in range(0, len(seq), width)),
                                "".join(qual[j:j + width] + "\n" for j in range(0, len(qual), width)))
        fq.append(rec)
        size += len(rec)
        i += 1
    return [("ragged_3000.fa", "".join(fa)), ("wraps_after_2MiB.fq", "".join(fq))]


def stream(path, strategy, batch_bases):
    """One run through a file: the summary line's fields."""
    from covest_amd import kmer_hist as kh
    digest, n_batches, reads, bases = hashlib.sha256(), 0, 0, 0
    try:
        rb = kh.ReadBatches(path, strategy, batch_bases=batch_bases, seed=3)
    except Exception as e:  # noqa: BLE001 -- the message is the result
        return "open failed: %s" % e
    failure = ""
    while True:
        got = rb._next()
        if isinstance(got, Exception):
            failure = " FAILED %s: %s" % (type(got).__name__, got)
            break
        ptr, offs, n, n_bases = got
        if n == 0:
            break
        digest.update(b"%d %d %d|" % (n, n_bases, rb.bytes_read))
        digest.update(ctypes.string_at(ptr, n_bases))
        digest.update(ctypes.string_at(offs, 8 * (n + 1)))
        n_batches, reads, bases = n_batches + 1, reads + n, bases + n_bases
    line = "batches %d reads %d bases %d bytes %d sha256 %s%s" % (n_batches, reads, bases, rb.bytes_read, digest.hexdigest(), failure)
    rb.close()
    return line


def dump(work, out_path):
    lines = []
    for name, text in small_shapes() + large_shapes():
        path = os.path.join(work, name)
        with open(path, "w", newline="") as f:
            f.write(text)
        for threads in THREADS:
            os.environ["COVEST_READER_THREADS"] = str(threads)  # (read by covest_reads_open)
            for strategy in (0, 1, 2):
                for batch_bases in BATCHES:
                    lines.append("%-34s threads %2d N %d batch %8d: %s" % (name, threads, strategy, batch_bases,
                                                                          stream(path, strategy, batch_bases)))
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def write_gigabase(path, fastq, n_reads=6_666_667, length=150):
    import numpy as np
    rng = np.random.default_rng(20240601)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    width = 3 + length + 1 + ((2 + length + 1) if fastq else 0)
    with open(path, "wb") as f:
        for a in range(0, n_reads, 500_000):
            n = min(500_000, n_reads - a)
            rec = np.empty((n, width), dtype=np.uint8)
            rec[:, :3] = np.frombuffer(b"@r\n" if fastq else b">r\n", dtype=np.uint8)
            rec[:, 3:3 + length] = lut[rng.integers(0, 4, size=(n, length), dtype=np.uint8)]
            rec[:, 3 + length] = 10
            if fastq:
                rec[:, 4 + length:6 + length] = np.frombuffer(b"+\n", dtype=np.uint8)
                rec[:, 6 + length:-1] = ord("I")
                rec[:, -1] = 10
            f.write(rec.tobytes())


def read_once(path):
    """(child) seconds to read the file through ReadBatches with its default batch, and what was read."""
    from covest_amd import _capi, kmer_hist as kh
    _capi.lib()
    t0 = time.perf_counter()
    reads = bases = 0
    for _, _, n, n_bases in kh.ReadBatches(path, kh.NS_IGNORE):
        reads, bases = reads + n, bases + n_bases
    print(json.dumps({"seconds": time.perf_counter() - t0, "reads": reads, "bases": bases}))


def child(lib, *args):
    env = dict(os.environ, COVEST_AMD_LIB=os.path.abspath(lib))
    return subprocess.run([sys.executable, os.path.abspath(__file__)] + list(args), env=env, timeout=1500, capture_output=True, text=True)


def time_ab(args, work):
    lines = ["# reading without counting, new library against the parent's (tools/compare_reads_libs.py --time): seconds of wall",
             "# time per pass over about 1 Gbase of 150-base reads, default threads and batch; one discarded pass, then five rounds,",
             "# the libraries alternating, every pass in a process of its own; accepted: new median <= parent's median * (1 + s),",
             "# s = (parent's max - min) / parent's median"]
    ok = True
    for fastq in (False, True):
        path = os.path.join(work, "gigabase.fq" if fastq else "gigabase.fa")
        write_gigabase(path, fastq, args.time_reads)
        times = {"parent": [], "new": []}
        for rnd in range(-1, 5):
            for tag, lib in (("parent", args.parent), ("new", args.new)):
                run = child(lib, "--read-once", path)
                if run.returncode != 0:
                    print(run.stdout + run.stderr)
                    return 1
                got = json.loads(run.stdout.strip().splitlines()[-1])
                print("%s round %d %s: %.3f s" % (os.path.basename(path), rnd, tag, got["seconds"]), file=sys.stderr, flush=True)
                if rnd >= 0:
                    times[tag].append(got["seconds"])
        os.remove(path)
        p, n = times["parent"], times["new"]
        s = (max(p) - min(p)) / statistics.median(p)
        accepted = statistics.median(n) <= statistics.median(p) * (1 + s)
        ok = ok and accepted
        lines += ["%s, %d reads, %d bases" % ("FASTQ" if fastq else "FASTA", got["reads"], got["bases"]),
                  "  parent  " + " ".join("%.3f" % t for t in p) + "   median %.3f  min %.3f  max %.3f  s %.3f" % (
                      statistics.median(p), min(p), max(p), s),
                  "  new     " + " ".join("%.3f" % t for t in n) + "   median %.3f  bound %.3f: %s" % (
                      statistics.median(n), statistics.median(p) * (1 + s), "accepted" if accepted else "NOT accepted")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out or os.path.join(REPO, "profiles", "reads_refactor_ab.txt"), "w") as f:
        f.write(text)
    return 0 if ok else 1


def digest_per_file(text, tag):
    """The record that is kept: the runs themselves are compared line by line above; per file of the corpus, how many
    runs, how many of them failed, a SHA-256 over the file's run lines, and each distinct failure."""
    by_file = {}
    for line in text.splitlines():
        by_file.setdefault(line.split()[0], []).append(line)
    out = ["# %s library: file, runs, failed, SHA-256 of its run lines; then the distinct failures" % tag]
    for name, lines in by_file.items():
        failures = sorted({line.split(" FAILED ", 1)[1] for line in lines if " FAILED " in line})
        out.append("%-34s %3d %3d %s" % (name, len(lines), sum(" FAILED " in line for line in lines),
                                         hashlib.sha256("\n".join(lines).encode()).hexdigest()))
        out += ["    %s" % f for f in failures]
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", nargs=2, metavar=("WORK", "OUT"), help="(child) stream the corpus with the library COVEST_AMD_LIB selects")
    ap.add_argument("--read-once", help="(child) time one pass over this file")
    ap.add_argument("--new")
    ap.add_argument("--parent")
    ap.add_argument("--work")
    ap.add_argument("--out")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--time-reads", type=int, default=6_666_667, help="reads per timed file (a smaller number rehearses --time)")
    args = ap.parse_args()
    if args.dump:
        dump(*args.dump)
        return 0
    if args.read_once:
        read_once(args.read_once)
        return 0
    work = args.work or tempfile.mkdtemp(prefix="reads_cmp_")
    os.makedirs(work, exist_ok=True)
    if args.time:
        return time_ab(args, work)
    outs = {}
    for tag, lib in (("new", args.new), ("parent", args.parent)):
        os.makedirs(os.path.join(work, tag), exist_ok=True)
        outs[tag] = os.path.join(work, tag + ".txt")
        run = child(lib, "--dump", os.path.join(work, tag), outs[tag])
        if run.returncode != 0:  # nothing more is started after a child that failed
            print("the %s library's run ended with status %d\n%s" % (tag, run.returncode, run.stdout + run.stderr))
            return 1
    with open(outs["new"]) as f:
        new = f.read()
    with open(outs["parent"]) as f:
        parent = f.read()
    differ = [i for i, (a, b) in enumerate(zip(new.splitlines(), parent.splitlines())) if a != b]
    head = "# the file front end, new library against the parent's (tools/compare_reads_libs.py): %d runs, %s\n" % (
        len(new.splitlines()), "the two outputs are the same file" if new == parent else "%d lines DIFFER" % max(len(differ), 1))
    for i in differ[:40]:
        print("new:    %s\nparent: %s" % (new.splitlines()[i], parent.splitlines()[i]))
    print(head, end="")
    with open(args.out or os.path.join(REPO, "profiles", "reads_refactor_cmp.txt"), "w") as f:
        f.write(head + digest_per_file(new, "new") + ("" if new == parent else digest_per_file(parent, "parent")))
    return 0 if new == parent else 1


if __name__ == "__main__":
    sys.exit(main())
