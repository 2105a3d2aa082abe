"""tests/seam_plan.py held to what it claims, with the oracle alone: every plant's byte where the plan says, the cross product of features
and seam phases complete, every text split (or refused, with the reference's message) by the oracle and given back by its decoder."""
import numpy as np
import pytest

import seam_plan as P

TEXTS = P.texts(0)
BY_NAME = {t.name: t for t in TEXTS}

# the byte(s) a feature is defined by, as the text must show them at the plant's offset (None: any letter / any byte of a name)
BYTES = {
    "fasta": {"gt": b">", "hdr_nl": b"\n", "id_space": b" ", "id_tab": b"\t", "acgt_hdr": b">", "hdr_1byte": b">", "lower1": b"acgt", "lower_first": b"acgt",
              "lower_last": b"acgt", "N": b"N", "R": b"R", "bang": b"!", "dash": b"-", "blank": b"\n", "crlf": b"\r", "cr": b"\r", "space": b" ", "tab": b"\t",
              "short_nl": b"\n", "long_nl": b"\n", "long5000": b"ACGT", "odd_last": b"ACGT", "end_nl": b"\n", "end_no_nl": b"ACGT",
              "stretch_lower_first": b"acgt", "stretch_lower_last": b"acgt"},
    "fastq": {"l0_first": b"@", "l1_first": b"ACGT", "l2_first": b"+", "l3_first": None, "l0_nl": b"\n", "l1_nl": b"\n", "l2_nl": b"\n", "l3_nl": b"\n", "id_space": b" ",
              "id_tab": b"\t", "no_comment": b"\n", "long_hdr_first": b"@", "long_hdr_blank": b" ", "qual_at": b"@", "qual_plus": b"+", "plus_name": None, "blank": b"\n",
              "crlf": b"\r", "space_seq": b" ", "bad_z": b"z", "iupac": b"R", "q01": b"\x01", "q7f": b"\x7f", "q80": b"\x80", "h01": b"\x01", "tab2": b"\t",
              "end_nl": b"\n", "end_no_nl": None},
}


def _context_ok(t, p):
    """What surrounds the defining byte, where one byte does not tell the feature."""
    d, x, f = t.data, p.offset, p.feature
    line0 = d.rfind(b"\n", 0, x) + 1
    line1 = d.find(b"\n", x)
    line1 = len(d) if line1 < 0 else line1
    if t.kind == "fasta":
        W = t.width
        if f in ("gt", "acgt_hdr", "hdr_1byte"):
            ok = line0 == x
            if f == "acgt_hdr": ok = ok and line1 - x > 2 * P.TILE and set(d[x + 1:line1]) <= set(b"ACGT")
            if f == "hdr_1byte": ok = ok and line1 == x + 1
            return ok
        if f in ("hdr_nl", "id_space", "id_tab"):
            return d[line0:line0 + 1] == b">" and (f == "hdr_nl" or d[line0:x].count(b" ") + d[line0:x].count(b"\t") == 0)
        if f in ("lower_first", "lower_last", "lower1", "stretch_lower_first", "stretch_lower_last"):
            # the letters around it, line ends apart: a run of exactly 300 lower-case bases that begins / ends there, or one alone
            before, after = d[max(0, x - 400):x].replace(b"\n", b""), d[x + 1:x + 400].replace(b"\n", b"")
            if f == "lower1": return before[-1:].isupper() and after[:1].isupper()
            if f.endswith("first"): return before[-1:].isupper() and after[:299].islower() and after[299:300].isupper()
            return after[:1].isupper() and before[-299:].islower() and before[-300:-299].isupper()
        if f == "blank": return d[x - 1] == 10
        if f == "crlf": return d[x + 1] == 10 and x - line0 == W
        if f == "cr": return d[x + 1] != 10 and x - line0 == W
        if f == "short_nl": return x - line0 == W - 1 and d[x + 1] != ord(">")
        if f == "long_nl": return x - line0 == W + 1
        if f == "long5000": return line0 == x and line1 - x == 5000 and x - 1 - (d.rfind(b"\n", 0, x - 1) + 1) == W
        if f == "odd_last":
            h = d.rfind(b">", 0, x)
            body = d[d.find(b"\n", h) + 1:x + 1]
            return d[x + 1] == 10 and d[x + 2:x + 3] == b">" and (len(body) - body.count(b"\n")) % 2 == 1
        if f in ("end_nl", "end_no_nl"): return x == len(d) - 1
        return True
    if f in ("l0_first", "long_hdr_first"): return line0 == x and (f == "l0_first" or line1 - x > P.TILE)
    if f == "long_hdr_blank": return d[line0:line0 + 1] == b"@" and line1 - line0 > P.TILE and b" " not in d[line0:x]
    if f in ("id_space", "id_tab"): return d[line0:line0 + 1] == b"@" and b" " not in d[line0:x] and b"\t" not in d[line0:x]
    if f == "no_comment": return d[line0:line0 + 1] == b"@" and b" " not in d[line0:x]
    if f in ("l1_first", "l2_first", "l3_first", "qual_at", "qual_plus"): return line0 == x
    if f == "plus_name": return d[line0:line0 + 1] == b"+" and line0 < x < line1 - 1
    if f == "blank": return d[x - 1] == 10
    if f == "tab2": return d[line0:x].count(b"\t") == 1
    if f in ("end_nl", "end_no_nl"): return x == len(d) - 1
    return True


@pytest.mark.parametrize("name", [t.name for t in TEXTS if t.family not in ("dying", "segments", "alignment")])
def test_plants_are_where_the_plan_says(name):
    t = BY_NAME[name]
    assert len(t.data) >= (288 if t.kind == "fasta" else 96) * 1024 - 1
    assert t.data[:2] == b"\n\n" and t.data[2:3] in b">@"                                          # blank lines in front of the first marker
    for p in t.plants:
        x, want = p.offset, BYTES[t.kind][p.feature]
        assert want is None or t.data[x] in want, (name, p, t.data[x - 4:x + 5])
        assert _context_ok(t, p), (name, p, t.data[x - 8:x + 9])
        seam = x - p.delta
        assert seam % p.unit == 0 and 0 < seam <= len(t.data) + 1, (name, p)          # (the end of a text one or two bytes in front of a seam)
        assert p.residues == (x % 4096, x % 64, x % 16) and p.residues[(P.TILE, P.LANE, P.PIECE).index(p.unit)] == p.delta % p.unit, (name, p)
        if p.unit == P.LANE: assert seam % P.TILE != 0, (name, p)
        if p.unit == P.PIECE: assert seam % P.LANE != 0, (name, p)
    body = t.plants[:-1]                                                                          # (the end of the text is where it is)
    assert all(b.offset - a.offset >= 3 * P.TILE for a, b in zip(body, body[1:])), (name, t.plants)
    assert body[0].offset - body[0].delta < 2 * P.TILE                                            # the first seam behind the first marker
    assert t.plants[-1].feature in P.END_FEATURES and t.plants[-1].offset == len(t.data) - 1      # the last whole seam before the end


def test_the_cross_product_is_complete(capsys):
    cp = P.cross_product()
    missing = sorted(k for k, v in cp.items() if v == 0)
    listed = {tuple(x[:4]) for x in P.IMPOSSIBLE}
    with capsys.disabled():
        print()
        for kind in ("fasta", "fastq"):
            feats = sorted({k[1] for k in cp if k[0] == kind})
            print("%s: plants of feature x (unit, delta)" % kind)
            print("%-16s" % "" + "".join("%8s" % ("%d%+d" % a) for a in P.ANCHORS))
            for f in feats:
                print("%-16s" % f + "".join("%8d" % cp[(kind, f, u, d)] for (u, d) in P.ANCHORS))
        print("cells %d, planted %d, impossible (listed with reasons) %d: %s" % (len(cp), len(cp) - len(missing), len(P.IMPOSSIBLE), P.IMPOSSIBLE))
    assert set(missing) == listed, missing
    assert all(len(x) == 5 and x[4] for x in P.IMPOSSIBLE)                                         # each with its reason
    assert len(P.IMPOSSIBLE) <= 0.02 * len(cp)


def test_plants_stay_where_they_are_under_other_seeds():
    for seed in (1, 2):
        for a, b in zip(TEXTS, P.texts(seed)):
            assert a.name == b.name and len(a.data) == len(b.data) and a.data != b.data
            assert [(p.feature, p.unit, p.delta, p.offset) for p in a.plants] == [(p.feature, p.unit, p.delta, p.offset) for p in b.plants]
            for p in b.plants:
                want = BYTES[b.kind].get(p.feature)
                assert want is None or b.data[p.offset] in want, (seed, b.name, p)


@pytest.mark.parametrize("count", P.SEGMENT_COUNTS)
def test_segment_count_tiles(count):
    t = BY_NAME["fq_segments_%d" % count]
    k = t.info["tile"]
    assert t.data[k * P.TILE:(k + 1) * P.TILE].count(b"\n") == count
    for j in (k - 1, k + 1, k + 2):                                                                # normal reads on both sides
        assert t.data[j * P.TILE:(j + 1) * P.TILE].count(b"\n") < 63


def test_stream_alignment_takes_every_residue(oracle):
    seen = {"seq": set(), "qual": set(), "ids": set(), "cmt": set()}
    for t in TEXTS:
        if t.family != "alignment":
            continue
        for p, (kind, j) in zip(t.plants, t.info["jobs"]):
            assert p.offset % P.TILE == 0 and t.data[p.offset:p.offset + 1] == b"@" and t.data[p.offset - 1] == 10
            sp = oracle.split_text(t.data[:p.offset])                                             # whole records: the streams in front of the tile
            got = {"seq": sp.n_bases, "qual": len(sp.qual), "ids": len(sp.ids), "cmt": len(sp.comments)}
            assert got[kind] % 16 == j, (t.name, p, got)
            seen[kind].add(got[kind] % 16)
            if kind == "seq":
                seen["qual"].add(got["qual"] % 16)
    assert all(v == set(range(16)) for v in seen.values()), seen


@pytest.mark.parametrize("name", [t.name for t in TEXTS])
def test_the_oracle_splits_or_refuses_every_text(oracle, name):
    t = BY_NAME[name]
    if t.dies:
        with pytest.raises(ValueError) as ei:
            oracle.split_text(t.data)
        assert t.dies in str(ei.value), (name, str(ei.value))
        return
    sp = oracle.split_text(t.data)
    want = t.decoded()                                                 # from the format's rules, not from the oracle
    assert sp.format == (oracle.FMT_FASTA if t.kind == "fasta" else oracle.FMT_FASTQ)
    marker = b">" if t.kind == "fasta" else b"@"
    assert sp.n_sequences == sum(1 for l in (want.split(b"\n")[::1 if t.kind == "fasta" else 4]) if l[:1] == marker) > 20
    feats = {p.feature for p in t.plants}
    if t.kind == "fasta":
        assert sp.longest_line == (5000 if "long5000" in feats else t.width + 1 if "long_nl" in feats else t.width), (name, sp.longest_line)
    assert oracle.unnaf(oracle.ennaf(t.data)) == want, name


def test_a_sample_splits_identically_under_the_live_reference(oracle, tmp_path):
    if not oracle.have_ref():
        pytest.skip("no reference binaries here")
    fams = {}
    for t in TEXTS:
        fams.setdefault((t.kind, t.family), t)
    for (kind, fam), t in fams.items():
        if t.dies:
            rc, _, err = oracle.ref_ennaf_full(t.data, tmpdir=str(tmp_path))
            assert rc != 0 and t.dies in err.decode("latin1"), (t.name, err)
            continue
        naf = oracle.ref_ennaf(t.data, tmpdir=str(tmp_path))
        assert oracle.ref_unnaf(naf) == oracle.unnaf(oracle.ennaf(t.data)) == t.decoded(), t.name
