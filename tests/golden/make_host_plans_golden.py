"""Golden for the host-side plans of liblcr_hip.so: every workspace size, the Sinkhorn form and lcr_kpconv_mask_ok over a small grid.

    python tests/golden/make_host_plans_golden.py

Recorded from a build of the commit BEFORE the workspace layouts, the Sinkhorn plan and the GEMM form predicate were each reduced to one
function (the parent of that change), with no LCR_* switch set in the environment: these numbers are a contract with every caller that
sizes a buffer, and with the byte offsets inside it, so a later change must reproduce them.  Needs the built library, no GPU — the
entries below only compute on the host.

The grid: the zero and one edge of every size argument, the shipped shapes (B = 1 and 16 pairs, 350 x 330 nodes, 128 x 128 patches), and
for Sinkhorn a (B, M, N) on each side of every form boundary:
  132 lines            (131, 131) register resident | (132, 131), (131, 132) LDS resident
  150 KiB of LDS       (192, 192) LDS resident      | (193, 193) beyond
  B * G = 64           (193, 193): B = 16 -> G = 4, B = 17 -> G = 2, B = 32 persistent | B = 33 per half-iteration launches
                       (350, 330): B = 10 -> G = 6, B = 11 -> G = 4, B = 16 persistent | B = 17 per half-iteration launches
  N + 1 > 1024         (2000, 1100): never persistent
  (1, 100)             register resident, yet its workspace is sized by the persistent form's hand-off buffers

Output: tests/golden/host_plans_golden.json — a list of [entry, [arguments], return code, value]."""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

SK_SHAPES = [(0, 1), (1, 0), (1, 1), (8, 8), (1, 100), (128, 128), (131, 131), (132, 131), (131, 132), (192, 192), (193, 193), (350, 330),
             (2000, 1100)]
SK_B = [0, 1, 10, 11, 16, 17, 32, 33]
MATCH_SHAPES = [(0, 1), (1, 0), (1, 1), (128, 128), (350, 330)]


def cases():
    """(entry, arguments) in a fixed order; entries that write through a pointer return their value, lcr_kpconv_mask_ok returns it directly"""
    out = []
    out += [("lcr_point_to_node_ws_bytes", [N, M]) for N in (0, 1, 1000, 120000, 32 * 120000) for M in (0, 1, 7, 350, 32 * 350)]
    for fn in ("lcr_top1_matching_ws_bytes", "lcr_topk_matching_ws_bytes"):
        out += [(fn, [B, M, N]) for B in (0, 1, 16, 3600) for M, N in MATCH_SHAPES]
    out += [("lcr_lgr_ws_bytes", [n, H, S]) for n in (0, 1, 5000, 200000) for H in (0, 1, 256, 4096) for S in (0, 1, 16)]
    out += [("lcr_netvlad_ws_bytes", [n, S]) for n in (0, 1, 350, 16 * 350) for S in (0, 1, 16)]
    out += [("lcr_retrieval_ws_bytes", [Q, C]) for Q in (-1, 0, 1, 2048, 2049, 4541) for C in (-1, 0, 1, 4541)]
    out += [("lcr_feature_nn_ws_bytes", [S, nq, nd]) for S in (0, 1, 16, 65536) for nq in (0, 1, 5000, 200000) for nd in (0, 1, 5000, 200000)]
    out += [("lcr_feature_correspondences_ws_bytes", [S]) for S in (0, 1, 16, 65535, 65536)]
    for fn in ("lcr_log_sinkhorn_ws_floats", "lcr_log_sinkhorn_form"):
        out += [(fn, [B, M, N]) for B in SK_B for M, N in SK_SHAPES]
    out += [("lcr_kpconv_mask_ok", [M, N, K, split]) for M, N, K, split in
            itertools.product((0, 1, 20000, 200000, 400000), (32, 64, 256), (240, 480, 960, 3840), (0, 1))]
    return out


def evaluate(L, entry, args):
    """(return code, value): the value an entry writes (None when it refuses), or lcr_kpconv_mask_ok's answer"""
    fn = getattr(L, entry)
    if entry == "lcr_kpconv_mask_ok":
        return 0, int(fn(*args))
    val = ctypes.c_int(-1) if entry == "lcr_log_sinkhorn_form" else ctypes.c_size_t(0)
    rc = int(fn(*args, ctypes.byref(val)))
    return rc, (int(val.value) if rc == 0 else None)


def main():
    from lcrnet_amd import _lib
    assert not [k for k in os.environ if k.startswith("LCR_")], "record with no LCR_* switch set"
    L = _lib.lib()
    rows = [[entry, args, *evaluate(L, entry, args)] for entry, args in cases()]
    with open(os.path.join(HERE, "host_plans_golden.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("%d rows" % len(rows))


if __name__ == "__main__":
    main()
