"""Selection of records and regions, the parts that need no GPU: the region grammar (naf_gpu_parse_region through ctypes) and the
command-line check that runs before the device is opened."""
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

BIN = os.path.join(ROOT, "naf_amd", "bin")


@pytest.mark.parametrize("text,want", [
    ("chr1", ("chr1", 0, None)),
    ("chr1:5-9", ("chr1", 4, 9)),
    ("chr1:5-", ("chr1", 4, None)),
    ("chr1:5", ("chr1", 4, 5)),
    ("chr1:1,000-2,000", ("chr1", 999, 2000)),
    ("a:b:3-4", ("a:b", 2, 4)),
    ("a:b", ("a:b", 0, None)),
    ("x:7-7", ("x", 6, 7)),
    ("sp|P1|X:12", ("sp|P1|X", 11, 12)),
])
def test_parse_region(text, want):
    from naf_amd import capi
    rid, b, e = capi.parse_region(text)
    assert (rid, b, e) == (want[0], want[1], capi.WHOLE if want[2] is None else want[2])
    assert capi.parse_region(text.encode()) == (rid.encode(), b, e)


@pytest.mark.parametrize("text", ["x:0-5", "x:9-3", "x:-4", "", ":5-9", "x:5--9", "x:5-9-", "x:,5", "x:99999999999999999999999-"])
def test_parse_region_rejects(text):
    from naf_amd import capi
    with pytest.raises(ValueError):
        capi.parse_region(text)


def test_region_is_in_the_c_abi():
    from naf_amd import capi
    lib = capi.load()
    for s in ("naf_gpu_unnaf_find", "naf_gpu_unnaf_record_table", "naf_gpu_unnaf_select_size", "naf_gpu_unnaf_select", "naf_gpu_parse_region"):
        assert s in capi.EXPORTS and hasattr(lib, s)


@pytest.mark.parametrize("args", [["--region", "x", "--ids"], ["--ids", "--records", "1-2"], ["--4bit", "--region", "x:1-5"], ["--charcount", "--region", "x"]])
def test_region_needs_sequence_output(args):
    naf = os.path.join(GOLDEN, "naf", "acgt_10k.naf")
    p = subprocess.run([os.path.join(BIN, "unnaf"), *args, naf], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b""
    assert p.stderr == b"unnaf error: --region can be used only with sequence output\n"


@pytest.mark.parametrize("args,msg", [(["--region", "x:0-5"], b"unnaf error: can't parse the value of --region parameter\n"),
                                      (["--records", "3-2"], b"unnaf error: can't parse the value of --records parameter\n"),
                                      (["--records", "0"], b"unnaf error: can't parse the value of --records parameter\n"),
                                      (["--records"], b"unnaf error: unknown or incomplete argument \"--records\"\n")])
def test_region_arguments_are_checked_on_the_command_line(args, msg):
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--fasta", *args], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 1 and p.stdout == b"" and p.stderr == msg


def test_help_keeps_the_reference_text_and_adds_the_selection_options():
    p = subprocess.run([os.path.join(BIN, "unnaf"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0
    ref_end = b"  -h, --help      - Show help\n  -V, --version   - Show version\n"
    head, sep, tail = p.stderr.partition(ref_end)
    assert sep and head.startswith(b"Usage: unnaf [OUTPUT-TYPE] [file.naf]\n") and b"--region" not in head and b"--records" not in head
    assert b"  --region " in tail and b"  --records " in tail
