"""CPU: the oracle restatement against the golden fixtures (reference flyweights via oracle/_ref,
tests/golden/*_ref.json) and the reference probe observations (SURVEY Appendix B,
tests/golden/survey_probes.json).  Bit-exact.  The expectations are golden_lib's, which
tests/test_gpu_golden.py runs with the device as subject."""
import os

import pytest

import golden_lib as G
import sbe_testlib as T
from golden_lib import load, probe_input  # noqa: F401 (survey_probes.json names probe_input as this module's)


@pytest.mark.parametrize("case", load("encode_ref.json")["cases"], ids=lambda c: str(c["ts"]))
def test_encode_matches_reference_flyweights(case):
    assert G.check_encode_ref([case], G.oracle_encode) == 1


@pytest.mark.parametrize("case", load("publish_ref.json")["cases"], ids=lambda c: str(c["ts"]))
def test_publish_topic_matches_reference_flyweights(case):
    """SBE_ENC_PUBLISH_TOPIC against ClusterClient::publish_topic's own flyweight sequence
    (src/cluster_client.cpp:1823-1858): lengths mod 65536, no E109."""
    assert G.check_publish_ref([case], G.oracle_encode) == 1


@pytest.mark.parametrize("case", load("decode_tm_ref.json")["cases"], ids=lambda c: c["name"])
def test_parse_tm_matches_reference_flyweights(case):
    assert G.check_parse_tm([case], G.oracle_decode) == 1


@pytest.mark.parametrize("case", load("ack_ref.json")["cases"], ids=lambda c: c["name"])
def test_decode_ack_matches_reference_flyweights(case):
    assert G.check_decode_ack([case], G.oracle_decode, to_nanos=T.oracle().orc_to_nanos_auto) == 1
    if not case["fails"]:  # the device tests use golden_lib's own statement of the conversion
        assert G.to_nanos_auto(int(case["ts"])) == int(T.oracle().orc_to_nanos_auto(int(case["ts"])))


@pytest.mark.parametrize("case", load("egress_tm_ref.json")["cases"], ids=lambda c: c["name"])
def test_on_egress_tm_matches_reference_flyweights(case):
    checked, claimed = G.check_egress_tm([case], G.oracle_decode)
    if claimed:
        pytest.skip("decode_ack claims this record first (checked in ack_ref)")
    assert checked == 1


def test_on_egress_tm_ack_claims():
    """How many egress_tm_ref cases decode_ack claims first with the oracle as subject: the device
    test may take that branch for no more."""
    cases = load("egress_tm_ref.json")["cases"]
    checked, claimed = G.check_egress_tm(cases, G.oracle_decode)
    assert claimed == G.EGRESS_TM_ACK_CLAIMED and checked + claimed == len(cases)


@pytest.mark.parametrize("probe", load("survey_probes.json")["probes"], ids=lambda p: p["name"])
def test_survey_probe(probe):
    G.check_survey_probe(probe, G.oracle_encode, G.oracle_decode)


def test_parse_ref_cases():
    """parse_ref.json: what the reference's compiled MessageParser::parse_message returned for the
    hand table of tests/refsrc_lib.py, all 17 ParseResult fields and the four predicates, with the
    oracle and the predicate model as subject.  The table itself is still the one the fixture was
    made from, and the fixture holds every outcome but the unreachable one."""
    import refsrc_lib as R
    cases = G.parse_ref_cases()
    assert [(c["name"], c["rec"]) for c in cases] == [(n, r.hex()) for n, r in R.hand_table()]
    assert G.check_parse_ref(cases, G.oracle_parse) == len(cases) >= 150
    seen = {R.outcome_class(G.unpack_result(c["result"])) for c in cases}
    assert seen == set(R.CLASSES) | {R.NULL_EMPTY}
    assert {c["pred"] for c in cases} >= {0, 1, 2, 6, 10, 14}
    assert os.path.getsize(os.path.join(G.GOLD, "parse_ref.json")) <= 32 * 1024
