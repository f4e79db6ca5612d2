"""The C boundary of gad_replay_relabel_goals (include/gaddpg.h section F: hindsight goals formed on the device): the ctypes mirror
against the real header, the export and plan tables, and every host-side refusal.  No GPU: nothing here launches."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NULL, ERR_SHAPE = -1, -2


def test_relabel_args_mirror_the_header():
    from ga_ddpg_amd import hip
    src = '#include "gaddpg.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu\\n", ' \
          'sizeof(gad_replay_relabel_args), sizeof(gad_replay_relabel_src), offsetof(gad_replay_relabel_args, row_start), ' \
          'offsetof(gad_replay_relabel_args, src), offsetof(gad_replay_relabel_args, idx), offsetof(gad_replay_relabel_args, end), ' \
          'offsetof(gad_replay_relabel_args, out_goal));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "p.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(d, "p")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(x) for x in subprocess.check_output([exe]).split()]
    A = hip.ReplayRelabelArgs
    assert got == [C.sizeof(A), C.sizeof(hip.ReplayRelabelSrc), A.row_start.offset, A.src.offset, A.idx.offset, A.end.offset,
                   A.out_goal.offset]
    assert C.sizeof(hip.ReplayRelabelSrc) == 16 and len(A().src) == hip.REPLAY_MAX_SRC


def test_relabel_entry_is_exported_and_plannable_under_abi_12():
    from ga_ddpg_amd import hip
    L = hip.lib()
    assert "gad_replay_relabel_goals" in hip.EXPORTS and hasattr(L, "gad_replay_relabel_goals")
    names = {L.gad_plan_entry_name(i).decode() for i in range(L.gad_plan_entry_count())}
    assert "gad_replay_relabel_goals" in names
    assert L.gad_abi_version() == 12


def _valid_args(hip, rows=(2, 3)):
    """arguments that pass every host-side check (dummy non-NULL addresses: never handed to a launch here)"""
    a = hip.ReplayRelabelArgs()
    a.B, a.n_src = sum(rows), len(rows)
    for s, r in enumerate(np.cumsum((0,) + tuple(rows))):
        a.row_start[s] = int(r)
    for s, n in enumerate(rows):
        if n:
            a.src[s].state_pose, a.src[s].expert_flags = 0x1000, 0x1000
    a.idx = a.end = a.out_goal = 0x1000
    return a


def test_relabel_goals_refuses_bad_arguments_before_any_launch():
    """every refusal is the ONLY defect of otherwise valid arguments, so each check is shown to exist; a status < 0 with a
    message that names the entry, and no launch (this runs without a GPU)"""
    from ga_ddpg_amd import hip
    L = hip.lib()
    null = C.c_void_p(None)

    def refused(a, status, word):
        rc = L.gad_replay_relabel_goals(C.byref(a), null)
        msg = L.gad_last_error()
        assert rc == status and b"replay_relabel_goals" in msg and word in msg, (rc, msg, word)

    rc = L.gad_replay_relabel_goals(null, null)
    assert rc == ERR_NULL and b"replay_relabel_goals" in L.gad_last_error()
    for n_src in (0, 5, -1):
        a = _valid_args(hip)
        a.n_src = n_src
        refused(a, ERR_SHAPE, b"n_src")
    for B in (0, -3, 65536):
        a = _valid_args(hip)
        a.B = B
        a.row_start[1] = a.row_start[2] = B
        refused(a, ERR_SHAPE, b"B ")
    a = _valid_args(hip)
    a.row_start[0] = 1
    refused(a, ERR_SHAPE, b"row_start")
    a = _valid_args(hip)
    a.row_start[2] = 4                                                 # does not end at B = 5
    refused(a, ERR_SHAPE, b"row_start")
    a = _valid_args(hip, rows=(2, 2, 1))
    a.row_start[1], a.row_start[2] = 3, 2                              # 0, 3, 2, 5: decreasing
    refused(a, ERR_SHAPE, b"decreases")
    for f in ("idx", "end"):
        a = _valid_args(hip)
        setattr(a, f, None)
        refused(a, ERR_NULL, b"index")
    a = _valid_args(hip)
    a.out_goal = None
    refused(a, ERR_NULL, b"output")
    for s in (0, 1):                                                   # a source that owns rows and relabels, without its flags
        a = _valid_args(hip)
        a.src[s].expert_flags = None
        refused(a, ERR_NULL, b"source %d" % s)
    a = hip.ReplayRelabelArgs()                                        # all zero: n_src = 0 is the first defect found
    refused(a, ERR_SHAPE, b"n_src")
