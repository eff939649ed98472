"""CPU: the image-list checks (ore_image_check_oriented, its NV12 and YUV forms and their non-oriented entries) answer
the table of _list_checks.py exactly as recorded in golden/list_check_messages.json: status, bad index and message,
byte for byte.  Where two rules are broken at once the message says which is tried first, so the recording pins the
order of the rules as well as their wording.  tools/record_list_checks.py made the recording from the library as it
was before the three checks shared one rule chain; nothing here rewrites it."""
import json
import os

import ore
from _list_checks import RULES, cases

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDING = os.path.join(HERE, "golden", "list_check_messages.json")


def test_table_is_the_recorded_one():
    with open(RECORDING) as f:
        rec = json.load(f)
    names = [name for name, _ in cases()]
    assert names == list(rec), "the table and the recording list different cases"
    assert 200 <= len(names) <= 900 and os.path.getsize(RECORDING) < 100 * 1024


def test_answers_match_the_recording():
    with open(RECORDING) as f:
        rec = json.load(f)
    L = ore.load()
    wrong = []
    for name, call in cases():
        got = call(L)
        if got != rec[name]:
            wrong.append(f"{name}: {got} != {rec[name]}")
    assert not wrong, "\n".join(wrong[:20])


def test_every_rule_alone_is_reached():
    """The recording itself: each rule broken alone fails and names its descriptor, at index 0 and at index 2, and
    no two rules of a format share a message."""
    with open(RECORDING) as f:
        rec = json.load(f)
    for fmt, rules in RULES.items():
        seen = set()
        for rule, _ in rules:
            for index in (0, 2):
                st, bad, msg = rec[f"{fmt}/{rule}@{index}"]
                assert st == 1 and bad == index and msg.startswith(f"image {index}: "), (fmt, rule, index, msg)
            body = rec[f"{fmt}/{rule}@0"][2]
            assert body not in seen, (fmt, rule, body)
            seen.add(body)
