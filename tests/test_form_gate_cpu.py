"""The form gate (qf.hpp: qf_form_faults, the body of k_validate_forms) on the host simulator, clause by clause against the
Python predicate of form_gate_cases, and the checks of the case table itself.  No GPU."""
import math

import pytest

import form_gate_cases as G
import simlib as S


@pytest.fixture(scope="module", params=["wg8", "wg32"])
def sim(request):
    return S.lib() if request.param == "wg8" else S.lib_wg32()


@pytest.mark.parametrize("i", range(5))
def test_simulator_reports_the_clauses_of_the_reference(sim, i):
    """every record of the table: the verdict word of the device predicate names exactly the clauses the Python predicate
    fails -- so a clause that is deleted, weakened or tested on the wrong lanes shows even where another clause would still
    refuse the record"""
    d = G.discriminants()[i]
    D = -d.delta
    got = S.validate([cs.rec for cs in d.cases], d.delta, sim)
    for cs, m in zip(d.cases, got):
        want = G.expected_mask(cs, D)
        assert m == want, "%s/%s: gate %s, reference %s" % (d.name, cs.label, [k for j, k in enumerate(G.CLAUSES) if m >> j & 1],
                                                           sorted(G.failed(cs.rec, D)))
        assert (m == 0) == (cs.names is None)


def test_the_table_has_the_five_discriminants():
    ds = G.discriminants()
    assert [d.name for d in ds] == ["tiny_k8", "s128_k128", "s128_k256", "odd_256", "owned_2400"]
    assert all(d.delta < 0 and d.delta % 4 in (0, 1) for d in ds)
    odd, own = ds[3], ds[4]
    assert odd.delta % 4 == 1 and (-odd.delta).bit_length() == 256
    assert (-own.delta).bit_length() == 2400 and (-G.too_wide_discriminant()).bit_length() == 2401
    labels = {cs.label for cs in own.cases}
    assert {"a_eq_c", "a_eq_c_negative", "b_eq_a", "b_eq_minus_a"} <= labels
    top_lane = 1 << (7 * G.LANE_BITS)
    assert any(cs.names is None and cs.rec[0] >= top_lane and cs.rec[1] >= top_lane for cs in own.cases), "data in the top lane"
    for d in ds[:3]:
        assert {"f", "h", "pk"} <= {cs.label for cs in d.cases}


def test_every_record_fits_a_record_and_labels_are_unique():
    for d in G.discriminants():
        assert len({cs.label for cs in d.cases}) == len(d.cases)
        for cs in d.cases:
            a, b, sw, c = cs.rec
            assert 0 <= a < G.PLANE and 0 <= b < G.PLANE and 0 <= c < G.PLANE ** 2 and 0 <= sw < 1 << 32, cs.label


def test_pass_records_fail_no_clause():
    for d in G.discriminants():
        assert len(G.passes(d)) >= 9
        for cs in G.passes(d):
            assert G.failed(cs.rec, -d.delta) == set(), (d.name, cs.label)
            f = G.as_form(cs.rec)
            assert f.disc() == d.delta and G.P.is_reduced(f), (d.name, cs.label)


def test_every_forgery_fails_exactly_the_clause_it_names():
    seen = set()
    for d in G.discriminants():
        for cs in G.forgeries(d):
            assert cs.names in G.CLAUSES
            bad = G.failed(cs.rec, -d.delta)
            if cs.label in G.EXCEPTIONS:
                seen.add(cs.label)
                assert {cs.names} <= bad <= {cs.names} | G.EXCEPTIONS[cs.label], (d.name, cs.label, sorted(bad))
            else:
                assert bad == {cs.names}, (d.name, cs.label, sorted(bad))
    assert seen == set(G.EXCEPTIONS) == {"a_zero", "c_zero", "all_max", "all_ones"}


def test_not_all_even_is_primitivity_on_the_whole_table():
    """the gate checks parity; the table says gcd.  They agree on every record but the listed one, so the table never claims
    more than the gate checks"""
    for d in G.discriminants():
        for cs in d.cases:
            a, b, _, c = cs.rec
            all_even = (a | b | c) & 1 == 0
            assert ((math.gcd(a, b, c) == 1) == (not all_even)) != (cs.label in G.PARITY_INEXACT), (d.name, cs.label)


def test_every_clause_is_isolated_in_three_discriminants():
    """a forgery that fails one clause and no other, in at least three of the five discriminants; `positive` and `no_carry`
    cannot be isolated (module docstring of the table): a forgery that names them, in at least three"""
    for clause in G.CLAUSES:
        hit = 0
        for d in G.discriminants():
            fs = [cs for cs in G.forgeries(d) if cs.names == clause]
            if clause in ("positive", "no_carry"):
                assert all(len(G.failed(cs.rec, -d.delta)) > 1 for cs in fs)
                hit += bool(fs)
            else:
                hit += any(G.failed(cs.rec, -d.delta) == {clause} for cs in fs)
        assert hit >= 3, clause


def test_near_misses_touch_every_lane_of_every_plane():
    """in the 2400-bit discriminant one forgery differs from a valid record by one bit in each of the 8 lanes of a, of |b| and
    of both planes of c, and nowhere else; in every discriminant each lane of c is covered"""
    def lanes(label_prefix, d, field, base):
        got = set()
        for cs in G.forgeries(d):
            if cs.label.startswith(label_prefix):
                diff = cs.rec[field] ^ base[field]
                assert diff and diff & (diff - 1) == 0 and all(cs.rec[k] == base[k] for k in range(4) if k != field), cs.label
                got.add((diff.bit_length() - 1) // G.LANE_BITS)
        return got

    for d in G.discriminants():
        by = {cs.label: cs.rec for cs in d.cases}
        assert lanes("c_bit_", d, 3, by["random0"]) == set(range(16)), d.name
        nb, na = lanes("b_bit_", d, 1, by["random0"]), lanes("a_bit_", d, 0, by["prime_form"])
        assert 0 in nb and 0 in na
        if d.name == "owned_2400":
            assert nb == set(range(8)) and na == set(range(8))
    for d in G.discriminants():
        w = {cs.label: cs.rec for cs in d.cases}["wrap_around"]
        assert w[0] * w[3] >= G.PLANE ** 2 and (w[1] ** 2 - d.delta) // 4 == w[0] * w[3] % G.PLANE ** 2


def test_wire_expressible_split():
    """what the GPU tier can send through the wire format and what only a record can say"""
    for d in G.discriminants():
        only_records = {cs.label for cs in d.cases if not G.on_wire(cs.rec)}
        assert only_records == {cs.label for cs in d.cases if cs.label.startswith("sign_word_") or cs.label in ("minus_zero", "a_zero", "c_zero")}
