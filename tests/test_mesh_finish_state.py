"""The bookkeeping of the indexed mesh's finish (voxelhashing_amd/csrc/vh_mesh_finish.hpp, VhMeshFinishState; DESIGN.md
section 4, "The finish as one chain") without a device: a stand-alone C++ program that includes the header's first part
alone, walks every sequence of up to four events and prints, after each event, the four stages' states and which stages
the inputs of the smoothing, the normals and the components pass through.  The print is compared with a restatement of
the design's table kept here."""
import itertools
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EVENTS = ("begin", "append", "cluster:0", "cluster:ok", "cluster:status", "smooth:0", "smooth:ok", "smooth:status", "normals", "components")
WELDED, CLUSTERED = 100, 40  # vertices of the welded mesh and of the clustered one

PROGRAM = r"""
#define VH_MESH_FINISH_STATE_ONLY
#include "vh_mesh_finish.hpp"
#include <cstdio>
#include <string>

static const char* kEvents[] = { %(events)s };
enum { kWelded = %(welded)d, kWeldedFaces = 190, kClustered = %(clustered)d, kClusteredFaces = 70, kDepth = 4 };

// what the chain's stage functions do to the state: start, (the pass), finish with the code its counts read back as
static void run(VhMeshFinishState& s, int stage, int code)
{
    s.start(stage);
    const bool clustered = stage > VH_FINISH_CLUSTER && (s.passes(stage - 1, kWelded) & 1u << VH_FINISH_CLUSTER) != 0;
    if (stage == VH_FINISH_CLUSTER) s.finish(stage, code, kClustered, kClusteredFaces);
    else if (stage == VH_FINISH_COMPONENTS) s.finish(stage, code, 0u, 0u);
    else s.finish(stage, code, clustered ? kClustered : kWelded, clustered ? kClusteredFaces : kWeldedFaces);
}
static void apply(VhMeshFinishState& s, int event)
{
    switch (event) {
    case 0: case 1: s.invalidateFrom(VH_FINISH_CLUSTER); break;
    case 2: s.forget(VH_FINISH_CLUSTER); break;
    case 3: run(s, VH_FINISH_CLUSTER, 0); break;
    case 4: run(s, VH_FINISH_CLUSTER, 2); break;
    case 5: s.forget(VH_FINISH_SMOOTH); break;
    case 6: run(s, VH_FINISH_SMOOTH, 0); break;
    case 7: run(s, VH_FINISH_SMOOTH, 4); break;
    case 8: run(s, VH_FINISH_NORMALS, 0); break;
    default: run(s, VH_FINISH_COMPONENTS, 0); break;
    }
}
static std::string stages(unsigned mask)
{
    std::string out;
    for (int s = 0; s < VH_FINISH_NUM_STAGES; s++)
        if (mask & 1u << s) out += "csnf"[s];
    return out;
}
static void walk(const VhMeshFinishState& before, const std::string& path, int depth)
{
    for (int e = 0; e < (int)(sizeof(kEvents) / sizeof(kEvents[0])); e++) {
        VhMeshFinishState s = before;
        apply(s, e);
        const std::string here = path.empty() ? kEvents[e] : path + " " + kEvents[e];
        std::string states;
        for (int g = 0; g < VH_FINISH_NUM_STAGES; g++) states += s.valid(g) ? 'V' : s.ran[g] ? 'r' : '-';
        std::printf("%%s | %%s | smooth<%%s normals<%%s components<%%s\n", here.c_str(), states.c_str(), stages(s.passes(VH_FINISH_CLUSTER, kWelded)).c_str(),
                    stages(s.passes(VH_FINISH_SMOOTH, kWelded)).c_str(), stages(s.passes(VH_FINISH_NORMALS, kWelded)).c_str());
        if (depth + 1 < kDepth) walk(s, here, depth + 1);
    }
}
int main()
{
    walk(VhMeshFinishState(), "", 0);
    return 0;
}
""" % dict(events=", ".join('"%s"' % e for e in EVENTS), welded=WELDED, clustered=CLUSTERED)

# ---- the table, restated: a stage is '-' (not run), 'r' (has run, and left a status) or 'V' (valid)
ORDER = ("cluster", "smooth", "normals", "components")
RESETS = {"begin": ORDER, "append": ORDER, "cluster": ORDER, "smooth": ORDER[1:], "normals": ("normals",), "components": ("components",)}


def vertices(state):
    return CLUSTERED if state["cluster"] == "V" else WELDED


def step(state, event):
    what, _, how = event.partition(":")
    if how == "0" and state[what] == "-":
        return  # switching off a pass that has not run changes nothing
    for stage in RESETS[what]:
        state[stage] = "-"
    if what in ORDER and how != "0":
        state[what] = "r" if how == "status" else "V"  # normals and components are valid even with a status: their queries report it
    if what == "normals":
        state["normals of"] = vertices(state)


def line(path, state):
    through = "".join(s[0] for s in ("cluster", "smooth") if state[s] == "V")  # the clustering's mesh, the smoothing's vertices
    rides = state["normals"] == "V" and state["normals of"] == vertices(state)
    return "%s | %s | smooth<%s normals<%s components<%s" % (" ".join(path), "".join(state[s] for s in ORDER), through.replace("s", ""), through,
                                                             through + ("n" if rides else ""))


def restated():
    out = []

    def walk(state, path):
        for event in EVENTS:
            s = dict(state)
            step(s, event)
            out.append(line(path + [event], s))
            if len(path) + 1 < 4:
                walk(s, path + [event])

    walk(dict(dict.fromkeys(ORDER, "-"), **{"normals of": 0}), [])
    return out


def test_every_sequence_of_up_to_four_events_follows_the_table():
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.cpp"), os.path.join(d, "t")
        open(src, "w").write(PROGRAM)
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-I", os.path.join(ROOT, "voxelhashing_amd", "csrc"), src, "-o", exe])
        got = subprocess.run([exe], stdout=subprocess.PIPE, check=True, timeout=60).stdout.decode().splitlines()
    want = restated()
    assert len(want) == sum(len(EVENTS) ** k for k in range(1, 5)) == len(got)
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    assert not wrong, "%d lines differ; the first (program, table): %r" % (len(wrong), wrong[0])
    # the walk is not vacuous: every state of every stage occurs, normals outlive a clustering nowhere, and somewhere the
    # components stay valid under new normals
    states = {l.split(" | ")[1] for l in want}
    assert {s[i] for s in states for i in (0, 1)} == {"-", "r", "V"} and {s[i] for s in states for i in (2, 3)} == {"-", "V"}
    assert any(l.startswith("components normals |") and l.split(" | ")[1] == "--VV" for l in want)
    assert any(l.endswith("components<csn") for l in want) and any(l.endswith("normals<s components<s") for l in want)
