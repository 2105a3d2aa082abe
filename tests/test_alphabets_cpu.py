"""tests/alphabet_plan.py held to what it claims, without a GPU: every plant's byte where the plan says, the cross product of features,
anchors, alphabets and formats complete, the models (decoded, unexpected, strict_verdict) against the oracle and -- where oracle/_ref is
built -- the real reference on every strict text, and each check of tests/test_gpu_alphabets.py rejecting a doctored expectation."""
import numpy as np
import pytest

import alphabet_plan as A
import seam_plan as P
from alphabet_plan import said, same_histograms, same_verdict

TEXTS = A.texts(0)
BY_NAME = {t.name: t for t in TEXTS}
STRICT_FAMILIES = ("strict", "numbered", "order", "strict_small")
ARGS = {A.DNA: (), A.RNA: ("--rna",), A.PROTEIN: ("--protein",), A.TEXT: ("--text",)}

# the byte(s) a feature is defined by (None: any letter / any byte of a name)
BYTES = {"gt": b">", "gt_line": b">", "hdr_1byte": b">", "hdr_nl": b"\n", "id_space": b" ", "id_tab": b"\t", "blank": b"\n", "crlf": b"\r", "cr": b"\r",
         "space": b" ", "tab": b"\t", "short_nl": b"\n", "long_nl": b"\n", "odd_last": None, "star": b"*", "dash": b"-", "lower1": b"acdefghiklmnpqrstvwy",
         "digit": b"7", "bang": b"!", "hi80": b"\x80", "hiFE": b"\xfe", "del7F": b"\x7f", "hiFF": b"\xff", "ctl01": b"\x01", "gt_mid": b">", "gt_in_id": b">",
         "l0_first": b"@", "l1_first": None, "l2_first": b"+", "l3_first": None, "l0_nl": b"\n", "l1_nl": b"\n", "l2_nl": b"\n", "l3_nl": b"\n",
         "qual_at": b"@", "qual_plus": b"+", "plus_name": None, "bad_seq": b"7\x7f", "q01": b"\x01", "q7f": b"\x7f", "q80": b"\x80", "space_seq": b" ",
         "end_nl": b"\n", "end_no_nl": None, "decoy": b"\x01!\x7f",
         "F_id": b"\xff", "F_comment": b"\xff", "F_seq": b"~\xff", "F_qual": b"\xff", "F_gt_in_id": b">", "F_seq_iupac": b"!"}
for _f in A.ID_FEATURES:
    BYTES[_f] = bytes([A.ID_BYTE[_f.split("_")[1]]])


def _line_of(d, x):
    a = max(d.rfind(b"\n", 0, x), d.rfind(b"\r", 0, x)) + 1
    e = [i for i in (d.find(b"\n", x), d.find(b"\r", x)) if i >= 0]
    return a, (min(e) if e else len(d))


def _context_ok(t, p):
    """What surrounds the defining byte, where one byte does not tell the feature."""
    d, x, f = t.data, p.offset, p.feature
    a, e = _line_of(d, x)
    marker = b">" if t.kind == "fasta" else b"@"
    if f in ("gt", "gt_line", "hdr_1byte", "l0_first"): return a == x and (f != "hdr_1byte" or e == x + 1) and (f != "gt_line" or d[d.rfind(b"\n", 0, a - 1) + 1] != 0x3E)
    if f in ("gt_mid",): return a < x and d[a] != 0x3E
    if f in ("gt_in_id", "F_gt_in_id", "F_id") or f in A.ID_FEATURES:
        ok = d[a:a + 1] == marker and b" " not in d[a:x] and b"\t" not in d[a:x]
        if f.endswith("_first"): ok = ok and x == a + 1
        if f.endswith("_last"): ok = ok and d[x + 1] in b" \t"
        if f in A.ID_FEATURES: ok = ok and b"\x01" in d[d.find(b" ", x):e]                      # cmt_ctl beside it
        return ok
    if f == "F_comment": return d[a:a + 1] == marker and b" " in d[a:x]
    if f in ("id_space", "id_tab"): return d[a:a + 1] == marker and b" " not in d[a:x] and b"\t" not in d[a:x]
    if f in ("F_seq", "F_seq_iupac", "bad_seq"): return d[a:a + 1] != marker or t.seq_type == A.TEXT
    if f == "blank": return d[x - 1] == 10
    if f == "crlf": return d[x + 1] == 10
    if f == "cr": return d[x + 1] != 10
    if f in ("end_nl", "end_no_nl"): return x == len(d) - 1
    return True


@pytest.mark.parametrize("name", [t.name for t in TEXTS if t.family in ("features", "ids", "strict")])
def test_plants_are_where_the_plan_says(name):
    t = BY_NAME[name]
    assert t.data[:2] == b"\n\n" and t.data[2:3] in b">@"                                          # blank lines in front of the first marker
    if t.seq_type <= A.RNA:
        assert len(t.data) >= 16 * P.TILE                                                          # the fast paths' floor
        assert t.kind == "fastq" or len(t.data) >> 17 >= 2                                          # and the one pass's under NAF_GPU_DIRECT=2
    for p in t.plants:
        x, want = p.offset, BYTES[p.feature]
        assert want is None or t.data[x] in want, (name, p, t.data[x - 4:x + 5])
        assert _context_ok(t, p), (name, p, t.data[x - 8:x + 9])
        assert p.residues == (x % 4096, x % 64, x % 16), (name, p)
        if p.note == "beside F":
            continue                                                                               # (a decoy beside F: F + 1, + 16, + 64)
        seam = x - p.delta
        assert seam % p.unit == 0 and 0 < seam <= len(t.data) + 1, (name, p)
        assert p.residues[(P.TILE, P.LANE, P.PIECE).index(p.unit)] == p.delta % p.unit, (name, p)
        if p.unit == P.LANE: assert seam % P.TILE != 0, (name, p)
        if p.unit == P.PIECE: assert seam % P.LANE != 0, (name, p)
    if t.family == "strict":
        F, decoys = t.plants[0], t.plants[1:]
        kind = {"id": 0, "gt_in_id": 0, "comment": 1, "seq": 2, "seq_iupac": 2, "qual": 3}[t.info["what"]]
        assert F.offset == t.info["first"] and [q.offset - F.offset for q in decoys[:3]] == [1, 16, 64]
        assert all(F.offset < q.offset and t.data[q.offset] < t.data[F.offset] for q in decoys), (name, t.plants)
        # the decoys in headers are bytes of an ID: kind 0, smaller than F's wherever a smaller kind exists
        assert all(_context_ok(t, P.Plant("F_id", q.unit, q.delta, q.offset)) for q in decoys[3:]), name
        assert kind >= 0 and decoys[-1].offset - F.offset >= 19 * P.TILE
        return
    body = t.plants[:-1]
    assert len(body) >= 2 and all(b.offset - a.offset >= 3 * P.TILE for a, b in zip(body, body[1:])), (name, t.plants)
    assert body[0].offset - body[0].delta < 2 * P.TILE                                             # the first seam behind the first marker
    assert t.plants[-1].feature in A.END_FEATURES and t.plants[-1].offset == len(t.data) - 1


def test_the_cross_product_is_complete(capsys):
    cp = A.cross_product()
    missing = sorted(k for k, v in cp.items() if v == 0)
    listed = {tuple(x[:6]) for x in A.IMPOSSIBLE}
    with capsys.disabled():
        print()
        for st in (A.DNA, A.RNA, A.PROTEIN, A.TEXT):
            for kind in ("fasta", "fastq"):
                for fam in ("features", "ids", "strict"):
                    feats = sorted({k[3] for k in cp if k[:3] == (st, kind, fam)})
                    if not feats:
                        continue
                    print("%s %s, %s: plants of feature x (unit, delta)" % (A.TYPE_NAME[st], kind, fam))
                    print("%-16s" % "" + "".join("%8s" % ("%d%+d" % a) for a in A.ANCHORS))
                    for f in feats:
                        print("%-16s" % f + "".join("%8d" % cp[(st, kind, fam, f, u, d)] for (u, d) in A.ANCHORS))
        print("cells %d, planted %d, impossible (listed with reasons) %d: %s" % (len(cp), len(cp) - len(missing), len(A.IMPOSSIBLE), A.IMPOSSIBLE))
    assert set(missing) == listed, missing
    assert all(len(x) == 7 and x[6] for x in A.IMPOSSIBLE)                                         # each with its reason
    assert len(A.IMPOSSIBLE) <= 0.05 * len(cp)
    assert not [x for x in A.IMPOSSIBLE if x[2] == "strict"]                                       # none in the strict families


def test_plants_stay_where_they_are_under_other_seeds():
    for seed in (1, 2):
        for a, b in zip(TEXTS, A.texts(seed)):
            assert a.name == b.name and len(a.data) == len(b.data), a.name
            assert a.family == "strict_small" or a.data != b.data, a.name
            assert [(p.feature, p.unit, p.delta, p.offset) for p in a.plants] == [(p.feature, p.unit, p.delta, p.offset) for p in b.plants]
            for p in b.plants:
                want = BYTES.get(p.feature)
                assert want is None or b.data[p.offset] in want, (seed, b.name, p)
            assert (A.strict_verdict(a.data, a.seq_type) is None) == (A.strict_verdict(b.data, b.seq_type) is None)


def test_record_numbers_in_front_of_the_offender():
    """300 headers and more in front of F, F - p0 on either side of 1, 2 and 3 blocks of the count, a header's '>' (and with it the line
    end in front of it) at -1, 0 and +1 of the count's 256-byte stride, blank lines and CR LF in front of a FASTQ's F, p0 of 0, 2 and 5."""
    seen = set()
    for t in TEXTS:
        if t.family != "numbered":
            continue
        d, X, p0 = t.data, t.info["first"], t.info["p0"]
        a = np.frombuffer(d[:X], dtype=np.uint8)
        marker = 0x3E if t.kind == "fasta" else 0x40
        starts = np.flatnonzero((a == marker) & (np.concatenate([[10], a[:-1]]) == 10))
        assert len(starts) >= 300 and starts[0] == p0 and set(d[:p0]) <= set(b"\t \n"), (t.name, len(starts), starts[:2])
        assert (X - p0) % A.BLOCK in (A.BLOCK - 1, 0, 1) and 1 <= round((X - p0) / A.BLOCK) <= 3, (t.name, X - p0)
        assert {254, 255, 0, 1, 2} <= set(((starts - p0) % 256).tolist()), t.name
        if t.kind == "fastq":
            assert b"\n\n@" in d[:X] and b"\r\n" in d[:X], t.name
        v = A.strict_verdict(d, t.seq_type, t.kind)
        n = len(starts) if t.kind == "fasta" else None
        assert v.startswith("unexpected %s code" % A.TYPE_NAME[t.seq_type]) and (n is None or v.endswith(" in sequence %d" % n)), (t.name, v)
        seen.add((t.kind, round((X - p0) / A.BLOCK), (X - p0 + 1) % A.BLOCK - 1, p0))
    assert {(k, b, dl) for (k, b, dl, _) in seen} == {(k, b, dl) for k in ("fasta", "fastq") for b in (1, 2, 3) for dl in (-1, 0, 1)}
    assert {p for (_, _, _, p) in seen} == {0, 2, 5}


def test_order_texts_end_their_record_on_the_seam():
    n = 0
    for t in TEXTS:
        if t.family != "order":
            continue
        x = t.plants[0].offset
        assert x - t.plants[0].delta == 3 * P.TILE and x < len(t.data)
        assert t.data[x] == 10 or x == len(t.data) - 1, (t.name, t.data[x - 3:x + 3])             # (a truncated record ends where it ends)
        assert x == len(t.data) - 1 or t.data[x + 1:x + 2] in (b"@", b"S"), (t.name, t.data[x:x + 4])   # ('S': the record lost its '@')
        n += 1
    assert n == len(A.ORDER_PLACES) * len(A.ORDER_DEATHS) * 9 + (4 * 3 + 3 + 2 + 2) * 3


@pytest.mark.parametrize("name", [t.name for t in TEXTS])
def test_the_models_against_the_oracle(oracle, name):
    """What the walk keeps, counts and stops at is what the oracle's split does; decoded() is what the oracle's decoder gives back."""
    t = BY_NAME[name]
    w = A.walk(t.data, t.seq_type)
    try:
        sp, err = oracle.split_text(t.data, t.seq_type), None
    except ValueError as e:
        sp, err = None, str(e).strip()
    assert err == w.stop, (name, err, w.stop)
    if err:
        assert t.family == "order"
        return
    assert sp.format == (oracle.FMT_FASTA if t.kind == "fasta" else oracle.FMT_FASTQ)
    assert sp.unexpected == A.unexpected(t.data, t.seq_type), name
    assert sp.ids == b"".join(i + b"\0" for i in w.ids) and sp.comments == b"".join(c + b"\0" for c in w.cmts), name
    assert sp.n_bases == len(w.stream) and sp.longest_line == w.longest and sp.n_sequences == w.n, name
    assert oracle.unnaf(oracle.ennaf(t.data, t.seq_type)) == t.decoded(), name
    if t.seq_type >= A.PROTEIN and t.family in ("features", "ids"):
        assert oracle.unnaf(oracle.ennaf(t.data, t.seq_type, True)) == A.decoded(t.data, t.seq_type, no_mask=True), name
    if t.family in ("features", "ids"):
        assert sum(sum(h) for h in sp.unexpected.values()) > 0 or t.family == "features", name
    if t.family == "ids":
        assert sum(sp.unexpected["id"]) == len(t.plants) - 1 and sum(sp.unexpected["comment"]) == len(t.plants) - 1, name


def test_a_sample_round_trips_under_the_live_reference(oracle, tmp_path):
    if not oracle.have_ref():
        pytest.skip("no reference binaries here")
    seen = {}
    for t in TEXTS:
        if t.family in ("features", "ids"):
            seen.setdefault((t.family, t.kind, t.seq_type), t)
    assert len(seen) == 12
    for t in seen.values():
        naf = oracle.ref_ennaf(t.data, ("--level", "1") + ARGS[t.seq_type], tmpdir=str(tmp_path))
        assert oracle.ref_unnaf(naf) == t.decoded(), t.name
        rc, _, err = oracle.ref_ennaf_full(t.data, ("--level", "1") + ARGS[t.seq_type], tmpdir=str(tmp_path))
        assert (rc, err.decode("latin1")) == (0, A.report(A.unexpected(t.data, t.seq_type), t.seq_type)), t.name


def test_strict_verdicts_against_the_live_reference(oracle, tmp_path, capsys):
    """The model's only independent witness: every strict text of seed 0 (and the clean ones, the seam texts and the 64 MiB text) through
    the real reference's --strict; status and stderr are the model's."""
    if not oracle.have_ref():
        pytest.skip("no reference binaries here")
    n = 0
    todo = [(t, t.seq_type) for t in TEXTS] + [(t, A.DNA) for t in A.seam_strict_texts(0)]
    for t, st in todo:
        v = A.strict_verdict(t.data, st)
        rc, _, err = oracle.ref_ennaf_full(t.data, ("--strict", "--level", "1") + ARGS[st], tmpdir=str(tmp_path))
        assert (rc, err.decode("latin1")) == ((1, "ennaf error: " + v + "\n") if v else (0, "")), (t.name, rc, err[:300], v)
        assert t.family not in STRICT_FAMILIES or v is not None, t.name
        n += 1
    data, v = A.big_text(0)
    rc, _, err = oracle.ref_ennaf_full(data, ("--strict", "--level", "1"), tmpdir=str(tmp_path))
    assert (rc, err.decode("latin1")) == (1, "ennaf error: " + v + "\n"), (rc, err[:300], v)
    with capsys.disabled():
        print("\nstrict texts held to the real reference: %d" % (n + 1))


def test_the_checks_reject_doctored_expectations():
    """A verdict that names the decoy, a record number off by one, a histogram with one count moved from ID to comment."""
    t = [x for x in TEXTS if x.family == "strict" and x.info["what"] == "seq" and x.kind == "fastq"][0]
    v = A.strict_verdict(t.data, t.seq_type)
    F = t.info["first"]
    healed = t.data[:F] + b"A" + t.data[F + 1:]
    decoy = A.strict_verdict(healed, t.seq_type)                                                    # what a key compared in the wrong order would name
    assert decoy is not None and decoy != v and "'!'" in decoy and "'~'" in v
    same_verdict(t, said("naf_gpu error 3: %s\n" % v), v)                                            # as the binding words a refusal
    with pytest.raises(AssertionError):
        same_verdict(t, said("naf_gpu error 3: %s\n" % decoy), v)
    with pytest.raises(AssertionError):
        same_verdict(t, "naf_gpu error 3: %s\n" % v, v)                                              # (the prefix is no part of the message)
    head, number = v.rsplit(" ", 1)
    for off in (-1, 1):
        with pytest.raises(AssertionError):
            same_verdict(t, "%s %d" % (head, int(number) + off), v)
    t = [x for x in TEXTS if x.family == "ids" and A.unexpected(x.data, x.seq_type)["id"][0x01]][0]
    want = A.unexpected(t.data, t.seq_type)
    same_histograms(t, want, want)
    moved = {k: list(h) for k, h in want.items()}
    moved["id"][0x01] -= 1; moved["comment"][0x01] += 1
    assert sum(sum(h) for h in moved.values()) == sum(sum(h) for h in want.values())
    with pytest.raises(AssertionError):
        same_histograms(t, moved, want)
