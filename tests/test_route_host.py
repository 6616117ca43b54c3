"""The two decisions of the operation-tree evaluator that pick device code (meryl_amd/csrc/mgc_route.hpp), pinned on a machine
without a GPU: a stand-alone host program built with the address and undefined-behaviour sanitizers runs eval_route over the full
grid of node kind x inputs x labels x program x assignment x MGC_MERGE_MANY and pass_inst over pass x program x program-asks-labels
x assignment x filter x output-labels, and both are compared with the tables written out here."""
import itertools
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY = None
MERGE, VALUE = 0, 1

# (kind, inputs, labels travel, node has a program, node has an assignment, MGC_MERGE_MANY enabled) -> route; the first row that
# matches decides
ROUTES = [
    # an assignment: merge_many with the ASSIGN rule, for both kinds (a value filter node under the presence rule of a union)
    ((ANY, ANY, ANY, ANY, 1, ANY), "many-assigned"),
    # a program: the SELECT forms, one input included
    ((VALUE, ANY, ANY, 1, 0, ANY), "select-selected"),
    ((MERGE, ANY, ANY, 1, 0, ANY), "many-selected"),
    # labels travel: plain count, labelled emit; every merge through merge_many whatever MGC_MERGE_MANY says, one input included
    ((VALUE, ANY, 1, 0, 0, ANY), "select-labelled"),
    ((MERGE, ANY, 1, 0, 0, ANY), "many-labelled"),
    # otherwise
    ((VALUE, ANY, 0, 0, 0, ANY), "select-plain"),
    ((MERGE, 3, 0, 0, 0, 1), "many-plain"),
    ((MERGE, 32, 0, 0, 0, 1), "many-plain"),
    ((MERGE, ANY, 0, 0, 0, ANY), "fold"),
]
MERGES_MANY = {"fold": 0, "select-plain": 0, "select-labelled": 0, "select-selected": 0, "many-plain": 1, "many-labelled": 1,
               "many-selected": 1, "many-assigned": 1}
CONTEXT = {"fold": "merging a slice", "many-plain": "merging a slice", "many-labelled": "merging a slice",
           "select-plain": "a value operation", "select-labelled": "a value operation",
           "select-selected": "a value operation with a selector", "many-selected": "merging a slice with a selector",
           "many-assigned": "merging a slice with a value assignment"}


def route_cases():
    """the full grid but what the evaluator's validation refuses before any route is taken: a value node has exactly one input; a
    merge of more than 32 inputs takes no labels, no program and no assignment.  (An assignment on an ARITHMETIC value node is
    refused too, but the route does not depend on the node's operation: the filter nodes stand for both here.)"""
    cases = []
    for kind, n, labels, program, assignment, many in itertools.product((MERGE, VALUE), (1, 2, 3, 32, 33), (0, 1), (0, 1), (0, 1), (0, 1)):
        if kind == VALUE and n != 1:
            continue
        if n == 33 and (labels or program or assignment):
            continue
        cases.append((kind, n, labels, program, assignment, many))
    return cases


def want_route(case):
    for pattern, route in ROUTES:
        if all(p is ANY or p == c for p, c in zip(pattern, case)):
            return route
    raise AssertionError(case)


def want_inst(emit, program, program_labels, assignment, filter_, out_labels):
    """(LABELS, SELECT, ASSIGN) of merge_many_kernel<K, EMIT, ...> (select_kernel: the same without ASSIGN)"""
    if not program and not assignment and not filter_:
        return (1 if emit and out_labels else 0, 0, 0)          # <K, false>; <K, true> or <K, true, true> by whether labels are written
    labels = 1 if program_labels or (emit and out_labels) else 0   # the program has a LABEL term (count), or that or labels written (emit)
    return (labels, 1, 1 if assignment or filter_ else 0)       # VOP_NONE without a filter is the selected case


def inst_cases():
    """the full grid but a LABEL term without anything that carries a program"""
    return [c for c in itertools.product((0, 1), repeat=6) if not (c[2] and not (c[1] or c[3] or c[4]))]


def test_route_and_instantiation_tables_on_the_host(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "route_host")
    c = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        os.path.join(ROOT, "tests", "host", "route_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr
    routes, insts = route_cases(), inst_cases()
    assert len(routes) == 2 * 8 * 4 + 2 + 8 * 2 and len(insts) == 64 - 4      # merge n <= 32, merge n = 33, value nodes
    lines = ["R %d %d %d %d %d %d" % c for c in routes] + ["I %d %d %d %d %d %d" % c for c in insts]
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got = p.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    seen = set()
    for case, g in zip(routes, got):
        want = want_route(case)
        assert g == "%s %d %s" % (want, MERGES_MANY[want], CONTEXT[want]), (case, g)
        seen.add(want)
    assert seen == set(CONTEXT)
    for case, g in zip(insts, got[len(routes):]):
        assert tuple(map(int, g.split())) == want_inst(*case), (case, g)
    # the instantiations the parent's launchers named, each reached: <K, false>, <K, true>, <K, true, true>, every
    # <K, EMIT, LABELS, true> and every <K, EMIT, LABELS, true, true>
    reached = {(c[0],) + want_inst(*c) for c in insts}
    assert reached == {(0, 0, 0, 0), (1, 0, 0, 0), (1, 1, 0, 0)} | {(e, l, 1, a) for e in (0, 1) for l in (0, 1) for a in (0, 1)}
