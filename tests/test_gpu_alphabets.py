"""The split pass in the modes tests/test_gpu_seams.py leaves out, on the texts of tests/alphabet_plan.py: the 8-bit alphabets (protein,
text: k_enc_count / k_enc_scatter<false>, k_encq_count / k_encq_scatter<false>) with their features at every seam phase; a damaged byte
in an ID, every alphabet, FASTA and FASTQ; and --strict -- the FIRST offender at every anchor with weaker decoys behind it, on every path
that has a sink of its own, its record counted across the blocks of k_count_starts, and ordered against a FASTQ's structural deaths
across a tile seam.  Every stream, histogram and decoded text against the oracle through check_ennaf; the histograms and the decoded text
also against the plan's own model, the refusal against the model's message (and the real reference's, where it is built).  No tolerance
anywhere: bytes, counts and messages are equal or the test fails.  tests/test_alphabets_cpu.py holds the plan and the models to their claims.

Letters, names and qualities are drawn for seeds 0, 1 and 2 (and moved further by NAF_TEST_SEED); the plants stay where they are."""
import os
import subprocess
import time

import pytest

import alphabet_plan as A
from test_gpu_encode import check_ennaf, host
from test_gpu_seams import same, where

pytestmark = pytest.mark.gpu
SEEDS = (0, 1, 2)
NAMES = A.names()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "naf_amd", "bin")
SWITCHES = {"fasta": (),
            "fastq": (("NAF_GPU_FQ_REG", "0"), ("NAF_GPU_FQ_FIRST", "0"), ("NAF_GPU_FQ_WAVE", "0"), ("NAF_GPU_FQ_FIRST", "check"))}
ARGS = {A.DNA: (), A.RNA: ("--rna",), A.PROTEIN: ("--protein",), A.TEXT: ("--text",)}
SMALL = b">after a refusal\nACGTNNacgt\nAC\n>second one\nGG\n"
SEAM_STRICT = [t.name for t in A.seam_strict_texts(0)]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    from naf_amd import capi
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def planned(name, seed):
    return A.texts(seed)[NAMES.index(name)]


def checked(gpu, O, t, **kw):
    try:
        return check_ennaf(gpu, O, t.data, **kw)
    except AssertionError as e:
        raise AssertionError("%s: %s\n%s" % (t.name, str(e)[:2000], where(gpu, O, t, t.data, kw))) from e


def histograms(rep):
    return {"id": list(rep.unexpected_id), "comment": list(rep.unexpected_comment), "seq": list(rep.unexpected_seq), "qual": list(rep.unexpected_qual)}


def kernels(gpu, call):
    """The names of the kernels that `call` launched, and what it returned (its exception is passed on)."""
    gpu.set_timing(True)
    gpu.get_timing()
    try:
        out = call()
    finally:
        names = {nm for nm, ms, k in gpu.get_timing()}
        gpu.set_timing(False)
    return names, out


def one_pass(t):
    """A 4-bit FASTA of 256 KiB and more: k_enc_fused reads it once under NAF_GPU_DIRECT=2 (enc.hip asks for 32 MiB otherwise)."""
    return t.kind == "fasta" and getattr(t, "seq_type", A.DNA) <= A.RNA and len(t.data) >> 17 >= 2


def said(e):
    return A.said(str(e.value))


def refused(gpu, t, verdict, seq_type, what=""):
    """gpu.ennaf(strict=True) raises exactly `verdict`."""
    from naf_amd.capi import NafGpuError
    with pytest.raises(NafGpuError) as e:
        gpu.ennaf(gpu.to_device(t.data), seq_type=seq_type, strict=True)
    A.same_verdict(t, said(e), verdict, what)


def under_every_switch(gpu, oracle, monkeypatch, t, verdict, seq_type):
    """The refusal on every path the text can take, the real reference where it is built, and a plain call directly behind the first
    refusal on the same context.  FASTQ: the default path and each of its switches.  A 4-bit FASTA of 256 KiB and more: the one pass
    (NAF_GPU_DIRECT=2, proved from the kernels launched), the two passes with direct blocks (NAF_GPU_ONEPASS=0, proved likewise) and
    without them (NAF_GPU_DIRECT=0).  Every other FASTA has one path, the general kernels: no switch changes it."""
    if one_pass(t):
        monkeypatch.setenv("NAF_GPU_PROBE", "0"); monkeypatch.setenv("NAF_GPU_DIRECT", "2")
        names, _ = kernels(gpu, lambda: refused(gpu, t, verdict, seq_type, "NAF_GPU_DIRECT=2"))
        assert "ennaf_split_once" in names and "ennaf_pure_check" in names, (t.name, sorted(names))
        check_ennaf(gpu, oracle, SMALL)
        monkeypatch.setenv("NAF_GPU_ONEPASS", "0")
        names, _ = kernels(gpu, lambda: refused(gpu, t, verdict, seq_type, "NAF_GPU_ONEPASS=0"))
        assert "ennaf_split_once" not in names and "ennaf_count_pure" in names, (t.name, sorted(names))
        monkeypatch.delenv("NAF_GPU_ONEPASS"); monkeypatch.setenv("NAF_GPU_DIRECT", "0")
        refused(gpu, t, verdict, seq_type, "NAF_GPU_DIRECT=0")
        monkeypatch.delenv("NAF_GPU_DIRECT"); monkeypatch.delenv("NAF_GPU_PROBE")
    refused(gpu, t, verdict, seq_type)
    check_ennaf(gpu, oracle, SMALL)
    for var, val in SWITCHES[t.kind]:
        monkeypatch.setenv(var, val)
        refused(gpu, t, verdict, seq_type, "%s=%s" % (var, val))
        monkeypatch.delenv(var)
    if oracle.have_ref():
        rc, _, err = oracle.ref_ennaf_full(t.data, ("--strict", "--level", "1") + ARGS[seq_type])
        assert (rc, err.decode("latin1")) == (1, "ennaf error: " + verdict + "\n"), (t.name, rc, err[:300], verdict)


# ---- A: the 8-bit alphabets and damaged IDs -----------------------------------------------------------------------------------------
def alphabet_checks(gpu, oracle, t):
    """check_ennaf; the report's histograms against the plan's own; the decoded text against the plan's own; returns the archive."""
    a = checked(gpu, oracle, t, seq_type=t.seq_type)
    d, rep = gpu.ennaf(gpu.to_device(t.data), seq_type=t.seq_type)
    same(t, a, host(d), "a second call")
    A.same_histograms(t, histograms(rep), A.unexpected(t.data, t.seq_type))
    assert oracle.unnaf(a, -1) == t.decoded(), (t.name, t.plants)
    if t.seq_type >= A.PROTEIN:
        # --no-mask upper-cases an 8-bit stream (the reference's seq_writer_nonmasked_text): the same archive where no letter is lower case
        b = checked(gpu, oracle, t, seq_type=t.seq_type, no_mask=True)
        s = bytes(A.walk(t.data, t.seq_type).stream)
        if s == s.upper():
            same(t, a, b, "no_mask")
        assert oracle.unnaf(b, -1) == A.decoded(t.data, t.seq_type, no_mask=True), (t.name, t.plants)
    return a


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", A.names("features"))
def test_alphabet_features_at_every_seam(gpu, oracle, name, seed):
    """Protein and text, FASTA and FASTQ: every tile through the general kernels in their 8-bit form."""
    alphabet_checks(gpu, oracle, planned(name, seed))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", A.names("ids"))
def test_damaged_ids_at_every_seam(gpu, oracle, monkeypatch, capfd, name, seed):
    """0x01, 0x7F and 0xFF at the first, a middle and the last byte of an ID, a control byte in the same header's comment: the byte is
    counted, dropped from the ID and a '?' enters the sequence stream.  The 4-bit FASTA texts are read ONCE (k_enc_fused, k_pure_check: the
    kernels launched say so) and hold one long record with a direct block and more; their archive is byte for byte the one of the two
    passes, and their streams are right without direct blocks.  The 4-bit FASTQ texts on the paths that must agree."""
    t = planned(name, seed)
    if t.seq_type > A.RNA:
        alphabet_checks(gpu, oracle, t)
        return
    if t.kind == "fasta":
        assert one_pass(t), (name, len(t.data))
        monkeypatch.setenv("NAF_GPU_PROBE", "0"); monkeypatch.setenv("NAF_GPU_DIRECT", "2"); monkeypatch.setenv("NAF_GPU_DEBUG_DIRECT", "1")
        capfd.readouterr()
        names, a = kernels(gpu, lambda: alphabet_checks(gpu, oracle, t))
        err = capfd.readouterr().err
        k = [int(l.split()[1]) for l in err.splitlines() if l.startswith("[direct]")]
        assert k and min(k) >= 1, (name, err[-300:])
        assert "ennaf_split_once" in names and "ennaf_pure_check" in names, (name, sorted(names))
        monkeypatch.delenv("NAF_GPU_DEBUG_DIRECT"); monkeypatch.setenv("NAF_GPU_ONEPASS", "0")
        names, b = kernels(gpu, lambda: checked(gpu, oracle, t, seq_type=t.seq_type))
        assert "ennaf_split_once" not in names and "ennaf_count_pure" in names, (name, sorted(names))
        same(t, a, b, "NAF_GPU_ONEPASS=0")
        monkeypatch.delenv("NAF_GPU_ONEPASS"); monkeypatch.setenv("NAF_GPU_DIRECT", "0")
        checked(gpu, oracle, t, seq_type=t.seq_type)
        return
    a = alphabet_checks(gpu, oracle, t)
    for var in ("NAF_GPU_FQ_REG", "NAF_GPU_FQ_FIRST", "NAF_GPU_FQ_WAVE"):
        monkeypatch.setenv(var, "0")
        same(t, a, host(gpu.ennaf(gpu.to_device(t.data), seq_type=t.seq_type)[0]), var + "=0")
        monkeypatch.delenv(var)
    monkeypatch.setenv("NAF_GPU_FQ_FIRST", "check")
    same(t, a, checked(gpu, oracle, t, seq_type=t.seq_type), "NAF_GPU_FQ_FIRST=check")


# ---- B: --strict ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", A.names("strict") + A.names("numbered") + A.names("order") + A.names("strict_small"))
def test_strict_names_the_first_offender(gpu, oracle, monkeypatch, name, seed):
    """The FIRST offender and not a decoy of a smaller byte and kind; the record's number behind 300 and more headers and on either side of
    a block of the header count; a strict byte against a structural death in the record in front, its own and the next."""
    t = planned(name, seed)
    verdict = A.strict_verdict(t.data, t.seq_type, t.kind)
    assert verdict is not None, name
    under_every_switch(gpu, oracle, monkeypatch, t, verdict, t.seq_type)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", SEAM_STRICT)
def test_strict_on_the_seam_texts(gpu, oracle, monkeypatch, name, seed):
    """The texts of seam_plan that hold an unexpected byte; the verdict is the model's.  The FASTA ones are read once under
    NAF_GPU_DIRECT=2 as in tests/test_gpu_seams.py, the FASTQ ones take the first look and the wave split by default."""
    t = [x for x in A.seam_strict_texts(seed) if x.name == name][0]
    verdict = A.strict_verdict(t.data, A.DNA, t.kind)
    assert verdict is not None and verdict.startswith("unexpected "), (name, verdict)
    under_every_switch(gpu, oracle, monkeypatch, t, verdict, A.DNA)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", A.names("clean"))
def test_strict_changes_nothing_of_a_clean_text(gpu, oracle, name, seed):
    t = planned(name, seed)
    assert A.strict_verdict(t.data, t.seq_type, t.kind) is None
    a = checked(gpu, oracle, t, seq_type=t.seq_type)
    same(t, a, host(gpu.ennaf(gpu.to_device(t.data), seq_type=t.seq_type, strict=True)[0]), "strict=True")


def test_strict_on_a_fresh_context(oracle):
    """The first call of a context is the refused one; the same refusal again; then a plain call.  One text of every family, format and
    alphabet (seed 0)."""
    from naf_amd import capi
    seen = {}
    for t in A.texts(0):
        if t.family in ("strict", "numbered", "order"):
            seen.setdefault((t.family, t.kind, t.seq_type, t.info.get("what")), t)
    assert len(seen) >= 30
    for t in seen.values():
        verdict = A.strict_verdict(t.data, t.seq_type, t.kind)
        ctx = capi.Context(0)
        try:
            refused(ctx, t, verdict, t.seq_type, "a fresh context")
            refused(ctx, t, verdict, t.seq_type, "a second refusal")
            check_ennaf(ctx, oracle, SMALL)
        finally:
            ctx.close()


def test_strict_behind_64_mib_of_headers(gpu, oracle):
    """F - p0 above 1024 * 65536: the header count's grid is clamped and strides.  The number comes from a numpy count.  A text of this
    size is read once by default (k_enc_fused).  The case may take five seconds; its smaller siblings are the numbered texts of three
    blocks."""
    from naf_amd.capi import NafGpuError
    data, verdict = A.big_text(0)
    d = gpu.to_device(data)

    def call():
        t0 = time.time()
        with pytest.raises(NafGpuError) as e:
            gpu.ennaf(d, strict=True)
        return e, time.time() - t0
    names, (e, dt) = kernels(gpu, call)
    print("64 MiB + 70 KiB under strict: %.3f s" % dt)
    assert said(e) == verdict
    assert "ennaf_split_once" in names and "ennaf_count_starts" in names, sorted(names)
    assert dt < 5.0, dt
    del d
    check_ennaf(gpu, oracle, SMALL)


@pytest.mark.parametrize("seq_type", (A.DNA, A.RNA, A.PROTEIN, A.TEXT))
@pytest.mark.parametrize("kind", ("fasta", "fastq"))
def test_the_command_line_reports_and_refuses(kind, seq_type):
    """naf_amd/bin/ennaf on one damaged-ID text per alphabet and format (seed 0): without --strict the report of unexpected characters on
    stderr and status 0, with it the model's message and status 1."""
    t = [x for x in A.texts(0) if x.family == "ids" and x.kind == kind and x.seq_type == seq_type][0]
    run = lambda *a: subprocess.run([os.path.join(BIN, "ennaf"), *a, *ARGS[seq_type], "-c"], input=t.data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    p = run()
    assert (p.returncode, p.stderr.decode("latin1")) == (0, A.report(A.unexpected(t.data, seq_type), seq_type)), (t.name, p.stderr[:400])
    p = run("--strict")
    assert (p.returncode, p.stderr.decode("latin1")) == (1, "ennaf error: " + A.strict_verdict(t.data, seq_type, kind) + "\n"), (t.name, p.stderr[:400])
