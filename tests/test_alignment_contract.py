"""
The alignment contract of include/fcdiff_hip.h against its tests and its documents: every (entry point, argument) that the
header's table requires to be 16-byte aligned is reached by a refusal parameter of tests/test_gpu_guard_bands.py, every
entry point that chooses its path by the address has its element-start test there, each of them says so in its own comment,
and INTEGRATION.md and the table of DESIGN.md list the same pairs.  CPU only; the table is read from the header's text, no
kernel is parsed.
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_arena as GA  # noqa: E402
import test_gpu_guard_bands as GB  # noqa: E402

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def read(*path):
    with open(os.path.join(ROOT, *path)) as fh:
        return fh.read()


def pairs(table):
    return sorted((ep, a) for (ep, args) in table.items() for a in args)


def test_the_parser_reads_the_table():
    text = "/*\n *   align16: fcd_a(x, y)     when T is even\n *   by-address: fcd_b(src)\n * align16 fcd_c(z)\n */\nint fcd_a(int x);"
    assert GA.alignment_contract(text) == ({"fcd_a": ["x", "y"]}, {"fcd_b": ["src"]})
    (a16, by) = GA.alignment_contract()
    assert len(a16) >= 16 and a16["fcd_gibbs_run"] == ["f_state", "lMf", "lMd"] and a16["fcd_corr_edges"] == ["ts"]
    assert sorted(by) == ["fcd_edge_cov_apply", "fcd_evidence_temper", "fcd_site_harmonize_apply"] and not set(by) & set(a16)


def test_every_listed_argument_is_reached_by_a_refusal():
    (a16, _by) = GA.alignment_contract()
    reached = set((ep, arg) for (_case, ep, arg, _buf) in GB.REFUSALS)
    missing = [p for p in pairs(a16) if p not in reached]
    assert not missing, "no refusal parameter of tests/test_gpu_guard_bands.py reaches: %s" % missing
    assert not reached - set(pairs(a16))
    # a parameter names a buffer of its case, and the reasons for leaving a pair out are written down
    for (case, ep, arg, buf) in GB.REFUSALS:
        spec = case.spec("small")
        assert ep in case.entry_points and (buf in spec["inputs"] or buf in spec["outputs"]), (case.name, ep, arg)
    for (key, reason) in GB.NOT_REFUSED_HERE.items():
        assert len(reason.split()) >= 5 and any(ep == key[1] for (_c, ep, _a, _b) in GB.REFUSALS), key
    # an emptied list of parameters is noticed
    assert [p for p in pairs(a16) if p not in set()] == pairs(a16)


def test_the_by_address_entry_points_have_their_element_start_tests():
    (_a16, by) = GA.alignment_contract()
    for ep in by:
        name = "test_%s_at_every_start" % ep[len("fcd_"):]
        assert callable(getattr(GB, name, None)), name
        assert '"%s"' % ep in read("tests", "test_gpu_guard_bands.py") or ep in read("tests", "test_gpu_harmonize.py")


def test_every_listed_entry_point_says_so_in_its_own_comment():
    text = read("include", "fcdiff_hip.h")
    (a16, by) = GA.alignment_contract(text)
    for (ep, args) in list(a16.items()) + list(by.items()):
        m = re.search(r"^int %s\(([^;]*)\);" % ep, text, flags=re.M)
        assert m, "%s is not a prototype of the header" % ep
        last = list(re.finditer(r"/\*.*?\*/", text[:m.start()], flags=re.S))[-1]
        own = last.group(0)
        assert text[last.end():m.start()].strip() == "", "%s has no comment of its own directly above it" % ep
        assert "Alignment:" in own, ep
        if ep in a16:
            assert "16-byte aligned" in own and all(re.search(r"\b%s\b" % a, own) for a in args), (ep, own[-200:])
            # the argument is a parameter of the prototype, or a member of the descriptor it takes
            for a in args:
                assert re.search(r"\b%s\b" % a, m.group(1)) or re.search(r"\*%s;" % a, text), (ep, a)
        else:
            assert "chosen by the address" in own, ep
    assert "FCD_ERR_ARG" in text[:text.index("#ifndef FCDIFF_HIP_H")] and "must be 16-byte aligned" in text


def table_pairs(md, heading):
    section = md[md.index(heading):]
    section = section[:section.index("\n## ", 1)]
    out = []
    for row in re.findall(r"^\| `(fcd_\w+)` \|([^\n]*)\|\s*$", section, flags=re.M):
        cells = row[1].split("|")
        out += [(row[0], a) for a in re.findall(r"`(\w+)`", cells[0])]
    return sorted(out)


def test_the_documents_list_the_same_pairs():
    (a16, by) = GA.alignment_contract()
    design = read("DESIGN.md")
    assert table_pairs(design, "## Alignment of caller pointers") == pairs(a16)
    integration = read("INTEGRATION.md")
    assert table_pairs(integration, "## Alignment of device pointers") == pairs(a16)
    for ep in by:
        assert "`%s`" % ep in design[design.index("## Alignment of caller pointers"):] and "`%s`" % ep in integration
    assert "FCD_ERR_ARG" in integration[integration.index("## Alignment of device pointers"):]
