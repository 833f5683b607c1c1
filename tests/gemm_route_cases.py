"""The leaves of the GEMM dispatcher (npvp_gemm_f32 -> eight kernel ids, their tile variants and split-K plans) and one table of
shapes that reaches every one of them at ragged edges.  Plain data + two pure helpers; tests/test_gemm_routes_host.py proves on
the CPU (npvp_gemm_route) that the table covers the dispatcher, tests/test_hip_gemm_routes.py runs every case on the GPU against
fp64.

A case is (name, mode, role, M, N, K, planes, leaf, expected route, options):
  mode    the GEMM arithmetic (ops.set_gemm_precision): f32 / f16x3 / bf16x6 / bf16x3
  role    "fwd"   y[M,N]  = x[M,K] w[N,K]^T      (a_kc, b_kc) = (1, 1)
          "dgrad" dx[M,N] = dy[M,K] w[K,N]       (1, 0)
          "wgrad" dw[M,N] = dy[K,M]^T x[K,N]     (0, 0): K = token rows
  planes  the weight's pre-split planes are handed over (ops._planes makes them from 256 token rows on)
  route   (kernel id, tile variant, split class, parity of the K-steps per split); split class: "1", "2..7", "x8" (a multiple of 8:
          the XCD remap), ">8" (above 8 and not a multiple of 8: plain block mapping); for the 128 x 128 kernels' pick_splits
          "1" / ">1"
"""

MODES = {"f32": 0, "bf16x6": 4, "bf16x3": 5, "f16x3": 6}
ROLES = {"fwd": (1, 1), "dgrad": (1, 0), "wgrad": (0, 0)}

# the bars of tests/test_hip_gemm_routes.py (and of tools/gemm_route_errors.py, which reads them here): whole-tensor rel-L2 per mode as
# test_gemm_full_size_against_rocblas, the worst row as close()'s ROW_TOL, frame statistics as test_linear_emits_frame_statistics
TOL = {"f32": 5e-5, "bf16x3": 5e-5, "bf16x6": 1e-5, "f16x3": 1e-5}
ROW_TOL = 1e-4
MEAN_TOL, RSTD_TOL = 1e-6, 2e-6

# leaf -> (kernel, (tile_m, tile_n), M can be ragged, N can be ragged)
LEAVES = {
    # ---- forward / dgrad
    "f32<1,1>":        ("gemm_f32_kernel<true,true>", (128, 128), True, True),
    "f32<1,0>":        ("gemm_f32_kernel<true,false>", (128, 128), True, True),
    "db3<1,1>":        ("gemm_split_db_kernel<3,true,true,false> (no planes)", (128, 128), True, True),
    "db3<1,0>":        ("gemm_split_db_kernel<3,true,false,false> (no planes)", (128, 128), True, True),
    # f16x3 with planes handed over but a shape the fp16 kernels decline (M < 128): the planes are dropped, bf16x6 on the fly.
    # Not reachable through linear_fwd / linear_dgrad (planes exist from 256 rows on, where gemm_f16_variant always takes the
    # shape): ops.gemm with b_pre given is the only way in
    "db3 planes dropped": ("gemm_split_db_kernel<3,true,*,false> (f16x3 planes ignored)", (128, 128), True, True),
    "db3<pre> fwd":    ("gemm_split_db_kernel<3,true,true,true> (F planes; gemm_wide declines)", (128, 128), True, True),
    "db3<pre> dgrad":  ("gemm_split_db_kernel<3,true,true,true> (D planes; gemm_wide declines)", (128, 128), True, True),
    "db2<1,1>":        ("gemm_split_db_kernel<2,true,true,false>", (128, 128), True, True),
    "db2<1,0>":        ("gemm_split_db_kernel<2,true,false,false>", (128, 128), True, True),
    "wide v1":         ("gemm_wide_kernel<2,4,2,2>", (128, 256), True, True),
    # wide_variant 2 requires N % 128 == 0: its column tiles are never ragged
    "wide v2":         ("gemm_wide_kernel<2,2,2,2>", (128, 128), True, False),
    "f16 v1":          ("gemm_f16_kernel<2,4,2,2,false>", (128, 256), True, True),
    # gemm_f16_variant 2 / 3 / 4 require N % 128 == 0; variant 3 exists only for M % 64 != 0; variant 4 requires M % 64 == 0 on
    # 64-row tiles: it has no ragged tile at all
    "f16 v2":          ("gemm_f16_kernel<2,2,2,2,false,2,3>", (128, 128), True, False),
    "f16 v3":          ("gemm_f16_kernel<2,1,2,2,false,2,3>", (128, 64), True, False),
    "f16 v4":          ("gemm_f16_kernel<1,2,2,2,false,2,3>", (64, 128), False, False),
    # rowstats needs M % 64 == 0 and N % 128 == 0: an odd frame count leaves the last 128-row tile half empty; N is ragged only
    # on the 256-column tiles of variant 1
    "f16 v1 rowstats": ("gemm_f16_kernel<2,4,2,2,true>", (128, 256), True, True),
    "f16 128x128 rowstats": ("gemm_f16_kernel<2,2,2,2,true,2,3> (what variants 2 / 3 / 4 run with rowstats)", (128, 128), True, False),
    # the same launches in bf16x6: the 128 x 128 kernel's rowstats instantiation splits B on the fly (it stages no planes), the
    # wide kernel has one per tile variant
    "db3 rowstats":    ("gemm_split_db_kernel<3,true,true,false,true>", (128, 128), True, False),
    "wide v1 rowstats": ("gemm_wide_kernel<2,4,2,2,true>", (128, 256), True, True),
    "wide v2 rowstats": ("gemm_wide_kernel<2,2,2,2,true>", (128, 128), True, False),
    # ---- weight gradients
    "f32<0,0> unsplit": ("gemm_f32_kernel<false,false>", (128, 128), True, True),
    "f32<0,0> split":   ("gemm_f32_kernel<false,false> + splitk_reduce_kernel", (128, 128), True, True),
    "db3<0,0> unsplit": ("gemm_split_db_kernel<3,false,false,false>", (128, 128), True, True),
    "db3<0,0> split":   ("gemm_split_db_kernel<3,false,false,false> + splitk_reduce_kernel", (128, 128), True, True),
    "db2<0,0> unsplit": ("gemm_split_db_kernel<2,false,false,false>", (128, 128), True, True),
    "db2<0,0> split":   ("gemm_split_db_kernel<2,false,false,false> + splitk_reduce_kernel", (128, 128), True, True),
    "wgrad wide 1":     ("gemm_wgrad_wide_kernel unsplit (512 or more tiles of 128 x 256: no layer of the model)", (128, 256), True, True),
    "wgrad wide x8":    ("gemm_wgrad_wide_kernel, splits % 8 == 0", (128, 256), True, True),
    "wgrad wide >8":    ("gemm_wgrad_wide_kernel, splits % 8 != 0", (128, 256), True, True),
    "wgrad f16 1":      ("gemm_wgrad_f16_kernel unsplit", (128, 256), True, True),
    "wgrad f16 2..7":   ("gemm_wgrad_f16_kernel, 2..7 splits", (128, 256), True, True),
    "wgrad f16 x8":     ("gemm_wgrad_f16_kernel, splits % 8 == 0", (128, 256), True, True),
    "wgrad f16 >8":     ("gemm_wgrad_f16_kernel, splits > 8 and % 8 != 0", (128, 256), True, True),
}

# the two hand-pipelined weight-gradient kernels unroll their K loop by two with a separate tail step: both parities of the
# K-steps per split must be reached, per kernel (kernel id -> name)
BOTH_PARITIES = {3: "gemm_wgrad_wide_kernel", 6: "gemm_wgrad_f16_kernel"}


def split_class(kernel_id, splits):
    if kernel_id in (0, 1):
        return "1" if splits == 1 else ">1"
    return "1" if splits == 1 else "2..7" if splits < 8 else "x8" if splits % 8 == 0 else ">8"


def leaf_of(mode, role, planes, rowstats, route):
    """the leaf a launch lands on, from its mode / role and the route npvp_gemm_route reports: (id, variant, splits, steps)"""
    kid, variant, splits, _ = route
    if role == "wgrad":
        if kid == 3:
            return "wgrad wide " + ("1" if splits == 1 else "x8" if splits % 8 == 0 else ">8")
        if kid == 6:
            return "wgrad f16 " + split_class(6, splits)
        base = {0: "f32<0,0>", 4: "db3<0,0>", 5: "db2<0,0>", 6: "db3<0,0>"}[MODES[mode]]
        return base + (" unsplit" if splits == 1 else " split")
    bk = "1,1" if role == "fwd" else "1,0"
    if kid == 0:
        return f"f32<{bk}>"
    if kid in (2, 4):
        return f"wide v{variant}" + (" rowstats" if rowstats else "")
    if kid in (5, 7):
        if rowstats:
            return "f16 v1 rowstats" if variant == 1 else "f16 128x128 rowstats"
        return f"f16 v{variant}"
    if mode == "bf16x3":
        return f"db2<{bk}>"
    if rowstats:
        return "db3 rowstats"
    if planes:
        return "db3 planes dropped" if mode == "f16x3" else f"db3<pre> {role}"
    return f"db3<{bk}>"


def _c(name, mode, role, M, N, K, planes, leaf, route, **opt):
    return dict(name=name, mode=mode, role=role, M=M, N=N, K=K, planes=planes, leaf=leaf, route=route, **opt)


# options: rowstats = the launch emits frame statistics (fwd only); adrop = also run the row-group mask on the rows of dy (f16x3 weight
# gradients; every dgrad case on the fp16 kernels runs it anyway)
CASES = [
    # ------------------------------------------------------------------ forward / dgrad, exact fp32
    _c("f32 fwd ragged", "f32", "fwd", 260, 136, 64, False, "f32<1,1>", (0, 0, "1", "even")),
    _c("f32 dgrad ragged", "f32", "dgrad", 260, 136, 64, False, "f32<1,0>", (0, 0, "1", "even")),
    # ------------------------------------------------------------------ three-term bf16, 128 x 128 tiles
    _c("db3 fwd no planes", "bf16x6", "fwd", 132, 72, 64, False, "db3<1,1>", (1, 0, "1", "even")),
    _c("db3 dgrad no planes", "bf16x6", "dgrad", 132, 72, 96, False, "db3<1,0>", (1, 0, "1", "even")),
    _c("db3 fwd no planes under f16x3", "f16x3", "fwd", 132, 72, 64, False, "db3<1,1>", (1, 0, "1", "even")),
    _c("db3 dgrad no planes under f16x3", "f16x3", "dgrad", 132, 72, 96, False, "db3<1,0>", (1, 0, "1", "even")),
    _c("f16x3 planes dropped fwd", "f16x3", "fwd", 68, 136, 64, True, "db3 planes dropped", (1, 0, "1", "even")),
    _c("f16x3 planes dropped dgrad", "f16x3", "dgrad", 68, 136, 64, True, "db3 planes dropped", (1, 0, "1", "even")),
    _c("db3 planes fwd ragged", "bf16x6", "fwd", 2080, 224, 96, True, "db3<pre> fwd", (1, 0, "1", "even")),
    _c("db3 planes dgrad ragged", "bf16x6", "dgrad", 2080, 224, 96, True, "db3<pre> dgrad", (1, 0, "1", "even")),
    _c("db3 planes fwd 20484 rows", "bf16x6", "fwd", 20484, 512, 64, True, "db3<pre> fwd", (1, 0, "1", "even")),
    _c("db3 planes dgrad 16420x1032", "bf16x6", "dgrad", 16420, 1032, 64, True, "db3<pre> dgrad", (1, 0, "1", "even")),
    # ------------------------------------------------------------------ two-term bf16
    _c("db2 fwd ragged", "bf16x3", "fwd", 2080, 224, 96, False, "db2<1,1>", (1, 0, "1", "even")),
    _c("db2 dgrad ragged", "bf16x3", "dgrad", 260, 136, 64, False, "db2<1,0>", (1, 0, "1", "even")),
    # ------------------------------------------------------------------ wide bf16 kernel
    _c("wide v1 fwd ragged", "bf16x6", "fwd", 6020, 2056, 64, True, "wide v1", (2, 1, "1", "even")),
    _c("wide v1 dgrad ragged", "bf16x6", "dgrad", 6020, 2056, 64, True, "wide v1", (2, 1, "1", "even")),
    _c("wide v2 fwd ragged rows", "bf16x6", "fwd", 2052, 512, 64, True, "wide v2", (4, 2, "1", "even")),
    _c("wide v2 dgrad 8200 rows", "bf16x6", "dgrad", 8200, 512, 96, True, "wide v2", (4, 2, "1", "even")),
    # ------------------------------------------------------------------ fp16 forward / dgrad
    _c("f16 v1 fwd ragged", "f16x3", "fwd", 2080, 224, 96, True, "f16 v1", (5, 1, "1", "even")),
    _c("f16 v1 dgrad ragged", "f16x3", "dgrad", 2080, 224, 96, True, "f16 v1", (5, 1, "1", "even")),
    _c("f16 v1 fwd 645 wide tiles", "f16x3", "fwd", 16420, 1032, 64, True, "f16 v1", (5, 1, "1", "even")),
    _c("f16 v2 fwd 8200 rows", "f16x3", "fwd", 8200, 512, 64, True, "f16 v2", (7, 2, "1", "even")),
    _c("f16 v2 dgrad 8200 rows", "f16x3", "dgrad", 8200, 512, 96, True, "f16 v2", (7, 2, "1", "even")),
    _c("f16 v3 fwd 2052 rows", "f16x3", "fwd", 2052, 512, 64, True, "f16 v3", (7, 3, "1", "even")),
    _c("f16 v3 dgrad 260 rows", "f16x3", "dgrad", 260, 128, 96, True, "f16 v3", (7, 3, "1", "even")),
    _c("f16 v3 fwd K 512", "f16x3", "fwd", 1056, 512, 512, True, "f16 v3", (7, 3, "1", "even")),
    _c("f16 v4 fwd", "f16x3", "fwd", 2048, 512, 64, True, "f16 v4", (7, 4, "1", "even")),
    _c("f16 v4 dgrad", "f16x3", "dgrad", 320, 128, 96, True, "f16 v4", (7, 4, "1", "even")),
    _c("f16 v1 rowstats 1025 frames", "f16x3", "fwd", 65600, 512, 64, True, "f16 v1 rowstats", (5, 1, "1", "even"), rowstats=True),
    _c("f16 v1 rowstats ragged columns", "f16x3", "fwd", 65600, 384, 64, True, "f16 v1 rowstats", (5, 1, "1", "even"), rowstats=True),
    _c("f16 128x128 rowstats 5 frames", "f16x3", "fwd", 320, 512, 64, True, "f16 128x128 rowstats", (7, 4, "1", "even"), rowstats=True),
    _c("f16 128x128 rowstats 129 frames", "f16x3", "fwd", 8256, 512, 64, True, "f16 128x128 rowstats", (7, 2, "1", "even"), rowstats=True),
    _c("db3 rowstats 1025 frames", "bf16x6", "fwd", 65600, 512, 64, True, "db3 rowstats", (1, 0, "1", "even"), rowstats=True),
    _c("wide v1 rowstats 97 frames", "bf16x6", "fwd", 6208, 2176, 64, True, "wide v1 rowstats", (2, 1, "1", "even"), rowstats=True),
    _c("wide v2 rowstats 5 frames", "bf16x6", "fwd", 320, 512, 64, True, "wide v2 rowstats", (4, 2, "1", "even"), rowstats=True),
    _c("wide v2 rowstats 129 frames", "bf16x6", "fwd", 8256, 512, 64, True, "wide v2 rowstats", (4, 2, "1", "even"), rowstats=True),
    # ------------------------------------------------------------------ weight gradients, 128 x 128 kernels (pick_splits)
    _c("f32 wgrad unsplit", "f32", "wgrad", 520, 264, 1056, False, "f32<0,0> unsplit", (0, 0, "1", "odd")),
    _c("f32 wgrad 5 splits", "f32", "wgrad", 520, 264, 2080, False, "f32<0,0> split", (0, 0, ">1", "odd")),
    _c("db3 wgrad unsplit", "bf16x6", "wgrad", 520, 264, 1056, False, "db3<0,0> unsplit", (1, 0, "1", "even")),
    _c("db3 wgrad 5 splits", "bf16x6", "wgrad", 520, 264, 2080, False, "db3<0,0> split", (1, 0, ">1", "even")),
    _c("db3 wgrad 7 splits", "bf16x6", "wgrad", 520, 264, 4256, False, "db3<0,0> split", (1, 0, ">1", "even")),
    _c("db2 wgrad unsplit", "bf16x3", "wgrad", 520, 264, 1056, False, "db2<0,0> unsplit", (1, 0, "1", "even")),
    _c("db2 wgrad 5 splits", "bf16x3", "wgrad", 520, 264, 2080, False, "db2<0,0> split", (1, 0, ">1", "even")),
    # ------------------------------------------------------------------ wide weight-gradient kernel (>= 32 768 token rows)
    _c("wgrad wide unsplit ragged", "bf16x6", "wgrad", 2052, 7944, 32768, False, "wgrad wide 1", (3, 0, "1", "even")),
    _c("wgrad wide 32 x 64 ragged", "bf16x6", "wgrad", 520, 264, 32768, False, "wgrad wide x8", (3, 0, "x8", "even")),
    _c("wgrad wide 64 x 33", "bf16x6", "wgrad", 512, 512, 33792, False, "wgrad wide x8", (3, 0, "x8", "odd")),
    _c("wgrad wide 41 x 50 ragged", "bf16x6", "wgrad", 520, 264, 32800, False, "wgrad wide >8", (3, 0, ">8", "even")),
    _c("wgrad wide 50 x 41", "bf16x6", "wgrad", 512, 512, 32800, False, "wgrad wide >8", (3, 0, ">8", "odd")),
    # ------------------------------------------------------------------ fp16 weight-gradient kernel (>= 1 024 token rows)
    _c("wgrad f16 unsplit ragged", "f16x3", "wgrad", 2052, 7944, 1056, False, "wgrad f16 1", (6, 0, "1", "even")),
    _c("wgrad f16 2 x 35 ragged", "f16x3", "wgrad", 520, 264, 1120, False, "wgrad f16 2..7", (6, 0, "2..7", "odd"), adrop=True),
    _c("wgrad f16 3 x 22 ragged", "f16x3", "wgrad", 520, 264, 1056, False, "wgrad f16 2..7", (6, 0, "2..7", "even")),
    _c("wgrad f16 5 x 26 ragged", "f16x3", "wgrad", 520, 264, 2080, False, "wgrad f16 2..7", (6, 0, "2..7", "even")),
    _c("wgrad f16 8 x 17 ragged", "f16x3", "wgrad", 520, 264, 2176, False, "wgrad f16 x8", (6, 0, "x8", "odd")),
    _c("wgrad f16 32 x 16 ragged", "f16x3", "wgrad", 520, 264, 8192, False, "wgrad f16 x8", (6, 0, "x8", "even")),
    _c("wgrad f16 14 x 19 ragged", "f16x3", "wgrad", 520, 264, 4256, False, "wgrad f16 >8", (6, 0, ">8", "odd")),
    _c("wgrad f16 41 x 50 ragged", "f16x3", "wgrad", 520, 264, 32800, False, "wgrad f16 >8", (6, 0, ">8", "even")),
    _c("wgrad f16 50 x 41", "f16x3", "wgrad", 512, 512, 32800, False, "wgrad f16 >8", (6, 0, ">8", "odd")),
]


def cases_for(mode):
    return [c for c in CASES if c["mode"] == mode]
