"""Generator of refusals.json: what unnaf writes to stderr, and its exit status, for a matrix of command lines of the table modes.

Every decision of unnaf's parse_command_line is taken before the input is opened, so with an input path that does not exist an accepted
command line ends in "can't open input file" and a refused one in its refusal, with or without a device.  The recording is of the
commit before the host's mode table; tests/test_host_cpu.py runs every case again and compares.  To check the fixture, build that
commit, run `python tests/golden/cli/make_refusals.py` and see an empty `git diff`.

This file only builds argument lists and runs the program."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
NO_INPUT = "no-such-directory/no-such-file.naf"
ACCEPTED = "unnaf error: can't open input file\n"

# a mode's name and the arguments that ask for it (locate in its plain and its bracketed form, runs in both its forms)
MODES = [("--locate", ["--locate", "NGG"]), ("--locate", ["--locate", "GAGTCC[NGG]"]), ("--composition", ["--composition"]), ("--quality", ["--quality"]),
         ("--runs", ["--runs", "N"]), ("--masked-runs", ["--masked-runs"]), ("--kmers", ["--kmers", "3"]), ("--orfs", ["--orfs"]),
         ("--translate", ["--translate"]), ("--repeats", ["--repeats", "misa"])]
MODE_NAMES = sorted({name for name, _ in MODES})
SATELLITES = [["--strand", "+"], ["--mismatches", "1"], ["--window", "100"], ["--cycles", "5"], ["--min-run", "2"], ["--each"], ["--canonical"],
              ["--per-record"], ["--min-orf", "30"], ["--stops", "TAA,TGA"], ["--starts", "ATG,GTG"], ["--stop-to-stop"], ["--closed"], ["--split-unknown"],
              ["--frame", "2,-1"], ["--code", "11"], ["--code-table", "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"],
              ["--min-repeat", "12"], ["--whole-units"]]
OTHERS = [["--fasta"], ["--ids"], ["--region", "x", "--revcomp"], ["--rc-region", "x"], ["--records", "1-2", "--records", "3-4"],
          ["--region", "x", "--records", "1"], ["--region", "x:1-5"], ["--region", "x"], ["--records", "2-3"], ["--no-mask"], ["--line-length", "60"]]
NUMBERS = [("--window", ["--composition"]), ("--cycles", ["--quality"]), ("--min-run", ["--runs", "N"]), ("--min-orf", ["--orfs"]), ("--min-repeat", ["--repeats", "misa"])]
VALUES = ["0", "", "x", "-1", "1e3", ",", "1,000", " 5", "9" * 20]
# what a mode checks for itself, and the pairs of satellites that the matrix above does not reach
OWN = [["--kmers", "7", "--per-record"], ["--kmers", "6", "--per-record"], ["--kmers", "7", "--per-record", "--fasta"], ["--kmers", "7", "--per-record", "--region", "x", "--revcomp"],
       ["--orfs", "--starts", "TAA"], ["--orfs", "--stops", "ATG"], ["--orfs", "--stop-to-stop", "--starts", "ATG"], ["--orfs", "--stop-to-stop", "--stops", "ATG"],
       ["--orfs", "--translate", "--frame", "2"], ["--orfs", "--translate", "--code", "11"], ["--orfs", "--translate", "--code", "11", "--starts", "TAG"],
       ["--orfs", "--translate", "--code", "6", "--starts", "TAA"], ["--orfs", "--translate", "--code-table", SATELLITES[16][1], "--stops", "ATG"],
       ["--orfs", "--translate", "--fasta"], ["--translate", "--orfs", "--region", "x", "--revcomp"], ["--orfs", "--translate", "--region", "x:1-5"],
       ["--orfs", "--translate", "--records", "1-2", "--records", "3-4"], ["--orfs", "--translate", "--repeats", "misa"], ["--orfs", "--translate", "--locate", "NGG"],
       ["--orfs", "--starts", "TAA", "--region", "x", "--revcomp"], ["--orfs", "--frame", "2", "--translate", "--revcomp", "--region", "x"],
       ["--translate", "--code", "11", "--code-table", SATELLITES[16][1]], ["--translate", "--code-table", SATELLITES[16][1], "--code", "11"],
       ["--translate", "--code", "11", "--code-table", SATELLITES[16][1], "--fasta"], ["--translate", "--code", "11", "--code-table", SATELLITES[16][1], "--composition"],
       ["--translate", "--rc-region", "x:1-5", "--region", "y", "--records", "1-2", "--revcomp"], ["--translate", "--frame", "6", "--region", "x:1-5"],
       ["--locate", "NGG", "--mismatches", "3"], ["--locate", "GAGTCC[NGG]", "--mismatches", "6"], ["--locate", "NGG", "--locate", "GAGTCC", "--mismatches", "3"],
       ["--mismatches", "3", "--locate", "NGG", "--fasta"], ["--locate", "NGG", "--mismatches", "1", "--mismatches", "2"], ["--mismatches", "9"],
       ["--runs", "N", "--masked-runs", "--locate", "NGG"], ["--masked-runs", "--runs", "N", "--fasta"], ["--runs", "N", "--runs", "A"], ["--runs", "N", "--each", "--masked-runs"],
       ["--masked-runs", "--each"], ["--quality", "--cycles", "5", "--composition", "--window", "3"], ["--window", "3", "--cycles", "5"],
       ["--revcomp"], ["--revcomp", "--composition"], ["--region", "x", "--ids"], ["--records", "1", "--revcomp", "--lengths"], ["-c", "-o", "out"],
       ["--locate", "NGG", "-c", "-o", "out"], ["--strand", "both", "--orfs", "--locate", "NGG"], ["--strand", "x"], ["--region", "x", "--fastq"]]


def cases():
    """The argument lists, without the input path, each once, in a fixed order."""
    out = []
    modes = [args for _, args in MODES]
    out += modes
    out += [a + b for a in modes for b in modes if a is not b]
    out += SATELLITES
    out += [x for s in SATELLITES for m in modes for x in (s + m, m + s)]
    out += [x for o in OTHERS for m in modes for x in (m + o, o + m)]
    out += [a + b + tail for i, a in enumerate(modes) for b in modes[i + 1:] for tail in (["--fasta"], ["--region", "x", "--revcomp"])]
    out += [m + s + tail for m in modes for s in SATELLITES for tail in (["--fasta"], ["--region", "x:1-5"])]
    out += [x for opt, mode in NUMBERS for v in VALUES for x in ([opt, v], mode + [opt, v])]
    out += OWN
    seen, once = set(), []
    for a in out:
        if tuple(a) not in seen:
            seen.add(tuple(a))
            once.append(list(a))
    return once


def run(unnaf, args):
    p = subprocess.run([unnaf, *args, NO_INPUT], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    return {"args": args, "status": p.returncode, "stdout": p.stdout.decode("latin1"), "stderr": p.stderr.decode("latin1")}


def run_all(unnaf, arg_lists):
    with ThreadPoolExecutor(8) as pool:
        return list(pool.map(lambda a: run(unnaf, a), arg_lists))


if __name__ == "__main__":
    unnaf = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "naf_amd", "bin", "unnaf")
    got = run_all(unnaf, cases())
    assert all(c["stdout"] == "" for c in got), "a case wrote to stdout"
    with open(os.path.join(HERE, "refusals.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps({k: c[k] for k in ("args", "status", "stderr")}) for c in got) + "\n]\n")
    print("%d cases, %d distinct messages, %d accepted" % (len(got), len({c["stderr"] for c in got}), sum(c["stderr"] == ACCEPTED for c in got)))
