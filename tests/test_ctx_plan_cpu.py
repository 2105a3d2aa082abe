"""The judges of the context tests can see (no GPU): every probe's reference agrees with a second, independent account of the same
input -- the oracle's text walked base by base, the oracle's own archive read back, a loop in plain Python --, every bait is an input the
oracle accepts and gives another result, and the pattern check names swapped, shifted, repeated and missing chunks."""
from collections import Counter

import numpy as np
import pytest

import composition_plan as CP
import ctx_plan as X
import kmers_plan as KP
import locate_near_plan as NP
import locate_plan as LP
import runs_plan as RP
import shard_standin


@pytest.fixture(scope="module")
def table(oracle):
    return X.by_name(oracle)


def test_the_table_names_every_family_once(table):
    assert len(table) == 20
    entries = {e for p in table.values() for e in p.entries}
    for e in ("zstd_compress", "zstd_decompress", "unnaf", "unnaf_size", "unnaf_range", "unnaf_select_stranded", "unnaf_find", "unnaf_record_table", "unnaf_locate",
              "unnaf_locate_near", "unnaf_composition", "unnaf_quality", "unnaf_runs", "unnaf_kmers", "unnaf_orfs", "ennaf", "ennaf_shard_begin", "ennaf_shard_finish",
              "ennaf_stitch", "histogram", "ennaf_count_lines"):
        assert "naf_gpu_" + e in entries, e
    for p in table.values():
        assert len(p.real) == len(p.bait) and p.real != p.bait, p.name


def test_references_of_the_texts_are_the_oracle_s(oracle, table):
    O = oracle
    naf_fa, naf_fq = table["unnaf_fasta"].real, table["unnaf_fastq"].real
    fa, fq = O.unnaf(naf_fa, 0), O.unnaf(naf_fq, 1)
    text = table["ennaf_overlap"].real
    assert fa == text                                                   # the archive is the oracle's of that very text
    assert table["unnaf_fasta"].ref(O) == ((len(fa),), fa) and table["unnaf_fastq"].ref(O) == ((len(fq),), fq)
    assert table["unnaf_size"].ref(O) == ((len(fa),), b"")
    assert table["unnaf_range"].ref(O) == ((4097,), fa[1003:1003 + 4097])
    # the selection and the tables, from the input text itself
    recs = [r.partition(b"\n") for r in text.split(b">")[1:]]
    ids = [h.split(b" ")[0] for h, _, _ in recs]
    bases = [b.replace(b"\n", b"") for _, _, b in recs]
    comp = bytes.maketrans(b"ACGTMRWSYKVHDBNacgtmrwsykvhdbn", b"TGCAKYWSRMBDHVNtgcakywsrmbdhvn")
    wrap = lambda s: b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60))
    want = (b">" + ids[1] + b":8-40\n" + bases[1][7:40] + b"\n" + b">" + ids[1] + b"/rc" + recs[1][0][len(ids[1]):] + b"\n" + wrap(bases[1].translate(comp)[::-1]) +
            b">" + ids[2] + b":6-%d/rc\n" % min(38, len(bases[2])) + bases[2][5:38].translate(comp)[::-1] + b"\n")
    assert table["unnaf_select_stranded"].ref(O) == ((len(want),), want)
    starts = np.concatenate([[0], np.cumsum([1 + len(h) + 1 + len(b) for h, _, b in recs])])
    assert table["unnaf_find_record_table"].ref(O)[0] == ((2, X.WHOLE, 0, len(recs) - 1), tuple(len(bases[r]) for r in (1, 2, 3)), tuple(int(starts[r]) for r in (1, 2, 3, 4)))
    # an archive read back by the oracle is the split of its text: what the ennaf probes hold the library's archive to
    for name in ("ennaf_overlap", "ennaf_shards"):
        host, streams = table[name].ref(O)
        assert X._streams(O, O.ennaf(text)) == streams and host == (len(recs), sum(len(b) for b in bases), 60)
    p = table["zstd_compress"]
    assert p.digest(O, O.zstd_store_raw(p.real)) == p.ref(O)[1] == p.real
    p = table["zstd_decompress"]
    assert p.ref(O)[1] == O.zstd_decompress(p.real) and len(p.ref(O)[1]) == p.cap and p.ref(O)[1] != p.reference(O, p.bait)[1]


def test_references_of_the_scanners_are_the_brute_force_s(oracle, table):
    O = oracle
    lines = X._lines(O, table["unnaf_fasta"].real)
    upper = [x.decode("latin1").upper() for x in lines]
    dt = lambda b, d: np.frombuffer(b, dtype=d)
    from naf_amd import capi
    (n,), out = table["unnaf_locate"].ref(O)
    rows = dt(out, capi.HIT_DTYPE)
    assert [(int(r["record"]), int(r["begin"]), int(r["pattern"]), int(r["strand"])) for r in rows] == sorted(LP.brute_hits(upper, ["ACG", "GRT"], 3)) and n == len(rows) > 100
    (n,), out = table["unnaf_locate_near"].ref(O)
    rows = dt(out, capi.NEAR_HIT_DTYPE)
    assert [tuple(int(r[f]) for f, _ in capi.NEAR_HIT_DTYPE) for r in rows] == sorted(tuple(t) for t in NP.brute_near(upper, ["ACGTAC[GT]", "TTNAGGC"], [1, 2], 3)) and n == len(rows) > 50
    (n, tot), out = table["unnaf_composition"].ref(O)
    rows = dt(out, capi.COMP_DTYPE)
    assert [(int(r["record"]), int(r["begin"]), int(r["end"]), tuple(int(v) for v in r["n"]), int(r["masked"]), int(r["cpg"])) for r in rows] == CP.brute_rows(lines, [100])[100]
    assert n == len(rows) and tot[2] == sum(len(x) for x in lines) and sum(tot[3]) == tot[2] and tot[4] > 0 and tot[5] > 0
    (n, nb), out = table["unnaf_runs"].ref(O)
    rows = dt(out, capi.RUN_DTYPE)
    assert RP.as_tuples(rows) == RP.brute_runs(lines, RP.set_of("ACGT"), each=True, min_len=3) and n == len(rows) > 50 and nb == sum(int(r["end"] - r["begin"]) for r in rows)
    (n, nc, tot), out = table["unnaf_kmers"].ref(O)
    counts = dt(out[:8 * nc], "<u8").reshape(n, 64)
    brute = KP.brute_counts(lines, 3, False, True)
    assert [{k: v for k, v in d.items() if v} for d in KP.as_dicts(counts, 3)] == [{k: v for k, v in d.items() if v} for d in brute]
    assert dt(out[8 * nc:], capi.KMER_DTYPE)["counted"].sum() == counts.sum() == tot[4] > 1000
    (n, nb), out = table["unnaf_orfs"].ref(O)
    rows = dt(out, capi.ORF_DTYPE)
    assert n == len(rows) > 20 and all((int(r["end"]) - int(r["begin"])) % 3 == 0 and int(r["end"]) - int(r["begin"]) >= 30 for r in rows)
    for r in rows[:40]:                                                 # an ORF from ATG reads ATG at its 5' end, and no stop inside
        s = upper[int(r["record"])][int(r["begin"]):int(r["end"])]
        s = s if not r["strand"] else LP.revcomp(s)
        assert s[:3] == "ATG" and not any(s[i:i + 3] in ("TAA", "TAG", "TGA") for i in range(0, len(s), 3)), (r, s[:9])
    (nr, ncy, hist, tot), out = table["unnaf_quality"].ref(O)
    fq = O.unnaf(table["unnaf_quality"].real, 1).split(b"\n")[3::4]
    assert nr == len(fq) == 100 and hist == [Counter(b"".join(fq)).get(v, 0) for v in range(256)] and tot[1] == sum(len(q) for q in fq) and tot[2] == sum(sum(q) for q in fq)
    rows = dt(out, capi.QUAL_DTYPE)
    assert [int(v) for v in rows["n"][:nr]] == [len(q) for q in fq] and int(rows["n"][nr:].sum()) == tot[1] and ncy == -(-max(len(q) for q in fq) // 16)


def test_line_starts_and_histogram_by_plain_loops(oracle, table):
    for name in ("count_lines_lf", "count_lines_crlf"):
        p = table[name]
        got = p.ref(oracle)[0][0]
        want = [len(shard_standin.line_starts(p.real if m is None else p.real[:m], bool(prev))) for m in X.LINE_SLICES for prev in (0, 1)]
        assert got == want and got[-1] == 6000 and got[2] in (0, 1)
    assert (b"\r\n" in table["count_lines_crlf"].real) and (b"\r" not in table["count_lines_lf"].real)
    p = table["histogram"]
    c = Counter(p.real)
    assert p.ref(oracle)[0][0] == [c.get(v, 0) for v in range(256)]


def test_every_bait_is_valid_input_with_another_result(oracle, table):
    for p in table.values():
        bait = p.reference(oracle, p.bait)                              # the oracle (or the plain reference) takes it
        real = p.ref(oracle)
        assert bait != real, p.name
        if p.cap and p.name not in ("zstd_compress",):
            assert bait[1] != real[1], p.name                           # and what lands in the output differs, not only a count
    p = table["zstd_compress"]
    assert oracle.zstd_decompress(oracle.zstd_store_raw(p.bait)) == p.bait != p.real


M = 1 << 20


def test_the_pattern_check_sees(oracle):
    n = 9 * M + 5
    good = X.pattern(n, 4097, 0x3C)
    assert X.pattern_diff(good, n, 4097, 0x3C) is None
    assert X.pattern_diff(good, n, 4096, 0x3C) is not None and X.pattern_diff(good, n, 4097, 0x3D) is not None
    swapped = good.copy()
    swapped[0:4 * M], swapped[4 * M:8 * M] = good[4 * M:8 * M], good[0:4 * M]
    msg = X.pattern_diff(swapped, n, 4097, 0x3C)
    assert msg and "byte 0 of" in msg and "%+d bytes away" % (4 * M) in msg, msg
    shifted = good.copy()
    shifted[4 * M:8 * M] = X.pattern(4 * M, 4097 + 4 * M + 1, 0x3C)
    msg = X.pattern_diff(shifted, n, 4097, 0x3C)
    assert msg and "byte %d of" % (4 * M) in msg and "+1 bytes away" in msg, msg
    twice = good.copy()
    twice[8 * M:] = good[4 * M:4 * M + M + 5]
    msg = X.pattern_diff(twice, n, 4097, 0x3C)
    assert msg and "byte %d of" % (8 * M) in msg and "%+d bytes away" % (-4 * M) in msg, msg
    msg = X.pattern_diff(good[:-3], n, 4097, 0x3C)
    assert msg and "short by 3" in msg, msg
    one = good.copy()
    one[n - 1] ^= 0x80
    msg = X.pattern_diff(one, n, 4097, 0x3C)
    assert msg and "byte %d of" % (n - 1) in msg and "1 in all" in msg, msg
    for shift in (1, 256, 4096, 4 * M, 8 * M, 16 * M, 64 * M):           # no shift a transfer could make leaves the bytes as they were
        assert not np.array_equal(X.pattern(4096, 0), X.pattern(4096, shift)), shift
