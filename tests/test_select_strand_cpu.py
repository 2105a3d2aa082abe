"""Reverse-complement selection, the parts that need no GPU: the new symbols, the command-line checks that run before the device is
opened, the help text, and the fact the device path rests on -- in the code table the complement of a code is the code with its
four bits reversed."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "naf_amd", "bin")


def test_stranded_select_is_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_unnaf_select_stranded_size", "naf_gpu_unnaf_select_stranded"):
        assert s in capi.EXPORTS and hasattr(lib, s)
    assert lib.naf_gpu_unnaf_select_stranded.argtypes is not None and len(lib.naf_gpu_unnaf_select_stranded.argtypes) == 10
    assert len(lib.naf_gpu_unnaf_select_stranded_size.argtypes) == 8


@pytest.mark.parametrize("out", ["--ids", "--4bit", "--charcount"])
@pytest.mark.parametrize("sel", [["--rc-region", "x"], ["--rc-region", "x:1-5"], ["--revcomp"], ["--revcomp", "--records", "1-2"], ["--revcomp", "--region", "x"]])
def test_reverse_complement_needs_sequence_output(out, sel):
    naf = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
    for args in ([out, *sel], [*sel, out]):
        p = subprocess.run([os.path.join(BIN, "unnaf"), *args, naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 1 and p.stdout == b""
        assert p.stderr == b"unnaf error: --region can be used only with sequence output\n"


@pytest.mark.parametrize("args,msg", [(["--revcomp"], b"unnaf error: --revcomp can be used only with --region or --records\n"),
                                      (["--rc-region", "x:0-5"], b"unnaf error: can't parse the value of --rc-region parameter\n"),
                                      (["--rc-region", "x:-4"], b"unnaf error: can't parse the value of --rc-region parameter\n"),
                                      (["--region", "x:-4"], b"unnaf error: can't parse the value of --region parameter\n"),
                                      (["--rc-region"], b"unnaf error: unknown or incomplete argument \"--rc-region\"\n")])
def test_strand_arguments_are_checked_on_the_command_line(args, msg):
    for first in (["--fasta"], []):
        p = subprocess.run([os.path.join(BIN, "unnaf"), *first, *args], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert p.returncode == 1 and p.stdout == b"" and p.stderr == msg


def test_help_lists_the_strand_options_behind_the_reference_text():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    ref_end = b"  -h, --help      - Show help\n  -V, --version   - Show version\n"
    head, sep, tail = p.stderr.partition(ref_end)
    assert sep and b"--rc-region" not in head and b"--revcomp" not in head
    assert b"  --rc-region " in tail and b"  --revcomp " in tail and b"  --region " in tail and b"  --records " in tail


@pytest.mark.parametrize("table,iupac_from,iupac_to", [("-TGKCYSBAWRDMHVN", "ACGTMRWSYKVHDBN-", "TGCAKYWSRMBDHVN-"),
                                                        ("-UGKCYSBAWRDMHVN", "ACGUMRWSYKVHDBN-", "UGCAKYWSRMBDHVN-")])
def test_the_complement_of_a_code_is_the_code_with_its_bits_reversed(table, iupac_from, iupac_to):
    assert len(table) == 16 and sorted(table) == sorted(iupac_from)
    tr = bytes.maketrans(iupac_from.encode(), iupac_to.encode())
    rev4 = lambda k: ((k & 1) << 3) | ((k & 2) << 1) | ((k & 4) >> 1) | (k >> 3)
    for k in range(16):
        assert table[rev4(k)] == table[k].encode().translate(tr).decode(), (k, table[k])
    assert "".join(table[rev4(k)] for k in range(16)) == ("-ACMGRSVTWYHKDBN" if "T" in table else "-ACMGRSVUWYHKDBN")
