"""The case table of the large-geometry tests of ``qs_mean_field`` and the two class keys it is measured by.

The host picks a launch geometry from (L, R, dtypes); ``qs_mean_field_plan`` reports it as numbers
``(Rc, nchunk, ct_log, ncb, nrb, lds_bytes, grid)``.  Two keys sort the geometries into the classes a kernel slip would
hit or miss as a whole:

  tile class   (ct_log, ncb > 1, nrb > 1, L odd)
  chunk class  (Rc capped by the LDS room for D, Rc == 1, nchunk == 1, short last chunk R % Rc != 0)

``CASES`` is explicit so that it can be read; tests/test_mean_field_cabi.py proves from the library's own plans that it
holds the smallest and the largest L of every tile class of every form over L = 1 ... 1024, every reachable chunk
class, and for every tile class with more than one column block a case with Rc > 1 and a short last chunk wherever the
size cap leaves one (else R >= 3).  tests/test_gpu_mean_field_geometry.py runs every case.

A case is (form, L, P, p_lo, R, r_lo): a slab of rows [p_lo, p_lo + P) and second indices [r_lo, r_lo + R) of an
(L, L, L, L) tensor, P * R * L * L <= 2^25 elements (a numpy.longdouble reference of at most 1 GiB).  The slab is
generated on its own: the kernel is told r_lo (it selects the columns of D) but never p_lo, which only names the rows
and seeds the generator.  This module imports neither torch nor the package under test."""

F64, C128 = 0, 1
PLAN_FIELDS = ("Rc", "nchunk", "ct_log", "ncb", "nrb", "lds_bytes", "grid")
MAX_ELEMENTS = 1 << 25

# form -> (u dtype code, D dtype code, cpi = columns per 16-byte item, dw = doubles per element of D and W)
FORMS = {"fp64": (F64, F64, 2, 1), "complex128": (C128, C128, 1, 2), "mixed": (F64, C128, 2, 2)}


def cdiv(a, b):
    return -(-a // b)


def tile_class(plan, L):
    """``plan``: the seven numbers of qs_mean_field_plan, in PLAN_FIELDS order."""
    p = dict(zip(PLAN_FIELDS, plan))
    return (p["ct_log"], p["ncb"] > 1, p["nrb"] > 1, L % 2 == 1)


def chunk_class(plan, L, R):
    """capped: the chunk length the target of 4096 work units asks for (include/qs_amd.h) did not fit the LDS room."""
    p = dict(zip(PLAN_FIELDS, plan))
    asked = cdiv(R, min(cdiv(4096, L), R))
    return (asked > p["Rc"], p["Rc"] == 1, p["nchunk"] == 1, R % p["Rc"] != 0)


def case_id(case):
    form, L, P, p_lo, R, r_lo = case
    return f"{form}-L{L}-P{P}@{p_lo}-R{R}@{r_lo}"


# the comment names what the library picks for the case (the CPU census recomputes it; it is not read by any test)
CASES = [
    ("fp64", 1, 1, 0, 1, 0),                # CT=128 ncb=1 nrb=1 Rc=1
    ("fp64", 15, 2, 8, 3, 6),               # CT=128 ncb=1 nrb=1 Rc=1
    ("fp64", 2, 2, 0, 2, 0),                # CT=128 ncb=1 nrb=1 Rc=1
    ("fp64", 16, 1, 7, 3, 3),               # CT=128 ncb=1 nrb=1 Rc=1
    ("fp64", 17, 2, 14, 3, 0),              # CT=64 ncb=1 nrb=1 Rc=1
    ("fp64", 31, 3, 8, 3, 26),              # CT=64 ncb=1 nrb=1 Rc=1
    ("fp64", 18, 1, 9, 3, 1),               # CT=64 ncb=1 nrb=1 Rc=1
    ("fp64", 32, 2, 20, 3, 7),              # CT=64 ncb=1 nrb=1 Rc=1
    ("fp64", 33, 3, 27, 3, 0),              # CT=32 ncb=1 nrb=1 Rc=1
    ("fp64", 63, 1, 2, 3, 46),              # CT=32 ncb=1 nrb=1 Rc=1
    ("fp64", 34, 2, 7, 3, 20),              # CT=32 ncb=1 nrb=1 Rc=1
    ("fp64", 64, 3, 17, 3, 56),             # CT=32 ncb=1 nrb=1 Rc=1
    ("fp64", 65, 1, 21, 65, 0),             # CT=64 ncb=1 nrb=3 Rc=2
    ("fp64", 127, 2, 92, 35, 66),           # CT=64 ncb=1 nrb=4 Rc=2
    ("fp64", 66, 3, 36, 65, 1),             # CT=64 ncb=1 nrb=3 Rc=2
    ("fp64", 128, 1, 106, 33, 76),          # CT=64 ncb=1 nrb=4 Rc=2
    ("fp64", 129, 2, 113, 33, 0),           # CT=128 ncb=1 nrb=9 Rc=2
    ("fp64", 255, 3, 120, 19, 86),          # CT=128 ncb=1 nrb=16 Rc=2
    ("fp64", 130, 1, 127, 33, 91),          # CT=128 ncb=1 nrb=9 Rc=2
    ("fp64", 256, 2, 134, 17, 96),          # CT=128 ncb=1 nrb=16 Rc=2
    ("fp64", 145, 3, 141, 31, 0),           # CT=32 ncb=3 nrb=3 Rc=2
    ("fp64", 959, 1, 148, 7, 106),          # CT=32 ncb=15 nrb=15 Rc=2
    ("fp64", 146, 2, 11, 31, 111),          # CT=32 ncb=3 nrb=3 Rc=2
    ("fp64", 960, 3, 162, 7, 116),          # CT=32 ncb=15 nrb=15 Rc=2
    ("fp64", 321, 1, 169, 15, 0),           # CT=64 ncb=3 nrb=11 Rc=2
    ("fp64", 895, 2, 176, 7, 126),          # CT=64 ncb=7 nrb=28 Rc=2
    ("fp64", 322, 3, 183, 15, 131),         # CT=64 ncb=3 nrb=11 Rc=2
    ("fp64", 896, 1, 190, 7, 136),          # CT=64 ncb=7 nrb=28 Rc=2
    ("fp64", 449, 2, 197, 11, 0),           # CT=128 ncb=2 nrb=29 Rc=2
    ("fp64", 1023, 3, 204, 7, 146),         # CT=128 ncb=4 nrb=64 Rc=2
    ("fp64", 450, 1, 211, 11, 151),         # CT=128 ncb=2 nrb=29 Rc=2
    ("fp64", 1024, 2, 218, 5, 156),         # CT=128 ncb=4 nrb=64 Rc=2
    ("fp64", 64, 1, 43, 64, 0),             # chunks: Rc=1 nchunk=64 CT=32 ncb=1 nrb=1
    ("fp64", 66, 2, 47, 66, 0),             # chunks: Rc=2 nchunk=33 CT=64 ncb=1 nrb=3
    ("fp64", 96, 3, 60, 65, 21),            # chunks: Rc=2 nchunk=33 CT=64 ncb=1 nrb=3
    ("fp64", 204, 1, 50, 204, 0),           # chunks: Rc=10 nchunk=21 CT=128 ncb=1 nrb=13
    ("fp64", 205, 2, 57, 204, 1),           # chunks: Rc=9 nchunk=23 CT=128 ncb=1 nrb=13
    ("fp64", 207, 3, 63, 207, 0),           # chunks: Rc=9 nchunk=23 CT=128 ncb=1 nrb=13
    ("fp64", 256, 1, 19, 256, 0),           # chunks: Rc=8 nchunk=32 CT=128 ncb=1 nrb=16
    ("fp64", 322, 1, 281, 322, 0),          # chunks: Rc=6 nchunk=54 CT=64 ncb=3 nrb=11
    ("fp64", 450, 1, 288, 165, 206),        # chunks: Rc=4 nchunk=42 CT=128 ncb=2 nrb=29
    ("fp64", 1024, 1, 295, 32, 211),        # chunks: Rc=2 nchunk=16 CT=128 ncb=4 nrb=64
    ("fp64", 1024, 2, 302, 1, 216),         # chunks: Rc=1 nchunk=1 CT=128 ncb=4 nrb=64
    ("complex128", 1, 1, 0, 1, 0),          # CT=128 ncb=1 nrb=1 Rc=1
    ("complex128", 15, 2, 8, 3, 6),         # CT=128 ncb=1 nrb=1 Rc=1
    ("complex128", 2, 2, 0, 2, 0),          # CT=128 ncb=1 nrb=1 Rc=1
    ("complex128", 16, 1, 7, 3, 3),         # CT=128 ncb=1 nrb=1 Rc=1
    ("complex128", 17, 2, 14, 3, 0),        # CT=64 ncb=1 nrb=1 Rc=1
    ("complex128", 31, 3, 8, 3, 26),        # CT=64 ncb=1 nrb=1 Rc=1
    ("complex128", 18, 1, 9, 3, 1),         # CT=64 ncb=1 nrb=1 Rc=1
    ("complex128", 32, 2, 20, 3, 7),        # CT=64 ncb=1 nrb=1 Rc=1
    ("complex128", 33, 3, 27, 3, 0),        # CT=64 ncb=1 nrb=2 Rc=1
    ("complex128", 63, 1, 2, 3, 46),        # CT=64 ncb=1 nrb=2 Rc=1
    ("complex128", 34, 2, 7, 3, 20),        # CT=64 ncb=1 nrb=2 Rc=1
    ("complex128", 64, 3, 17, 3, 56),       # CT=64 ncb=1 nrb=2 Rc=1
    ("complex128", 65, 1, 21, 65, 0),       # CT=128 ncb=1 nrb=5 Rc=2
    ("complex128", 127, 2, 92, 35, 66),     # CT=128 ncb=1 nrb=8 Rc=2
    ("complex128", 66, 3, 36, 65, 1),       # CT=128 ncb=1 nrb=5 Rc=2
    ("complex128", 128, 1, 106, 33, 76),    # CT=128 ncb=1 nrb=8 Rc=2
    ("complex128", 129, 2, 113, 33, 0),     # CT=64 ncb=3 nrb=5 Rc=2
    ("complex128", 959, 3, 120, 3, 86),     # CT=64 ncb=15 nrb=30 Rc=1
    ("complex128", 130, 1, 127, 33, 91),    # CT=64 ncb=3 nrb=5 Rc=2
    ("complex128", 960, 2, 134, 3, 96),     # CT=64 ncb=15 nrb=30 Rc=1
    ("complex128", 193, 3, 141, 23, 0),     # CT=8 ncb=25 nrb=1 Rc=2
    ("complex128", 247, 1, 148, 19, 106),   # CT=8 ncb=31 nrb=1 Rc=2
    ("complex128", 194, 2, 155, 23, 111),   # CT=8 ncb=25 nrb=1 Rc=2
    ("complex128", 248, 3, 162, 19, 116),   # CT=8 ncb=31 nrb=1 Rc=2
    ("complex128", 201, 1, 169, 23, 0),     # CT=128 ncb=2 nrb=13 Rc=2
    ("complex128", 1023, 2, 176, 3, 126),   # CT=128 ncb=8 nrb=64 Rc=1
    ("complex128", 202, 3, 183, 23, 131),   # CT=128 ncb=2 nrb=13 Rc=2
    ("complex128", 1024, 1, 190, 3, 136),   # CT=128 ncb=8 nrb=64 Rc=1
    ("complex128", 449, 2, 197, 11, 0),     # CT=8 ncb=57 nrb=2 Rc=2
    ("complex128", 1015, 3, 204, 3, 146),   # CT=8 ncb=127 nrb=4 Rc=1
    ("complex128", 450, 1, 211, 11, 151),   # CT=8 ncb=57 nrb=2 Rc=2
    ("complex128", 1016, 2, 218, 3, 156),   # CT=8 ncb=127 nrb=4 Rc=1
    ("complex128", 64, 1, 43, 64, 0),       # chunks: Rc=1 nchunk=64 CT=64 ncb=1 nrb=2
    ("complex128", 66, 2, 47, 66, 0),       # chunks: Rc=2 nchunk=33 CT=128 ncb=1 nrb=5
    ("complex128", 96, 3, 60, 65, 21),      # chunks: Rc=2 nchunk=33 CT=128 ncb=1 nrb=6
    ("complex128", 158, 1, 96, 157, 0),     # chunks: Rc=6 nchunk=27 CT=64 ncb=3 nrb=5
    ("complex128", 162, 2, 100, 162, 0),    # chunks: Rc=6 nchunk=27 CT=64 ncb=3 nrb=6
    ("complex128", 248, 2, 21, 248, 0),     # chunks: Rc=4 nchunk=62 CT=8 ncb=31 nrb=1
    ("complex128", 322, 1, 274, 322, 0),    # chunks: Rc=3 nchunk=108 CT=128 ncb=3 nrb=21
    ("complex128", 450, 1, 281, 165, 0),    # chunks: Rc=2 nchunk=83 CT=8 ncb=57 nrb=2
    ("complex128", 512, 1, 288, 128, 206),  # chunks: Rc=2 nchunk=64 CT=128 ncb=4 nrb=32
    ("complex128", 513, 1, 295, 127, 211),  # chunks: Rc=1 nchunk=127 CT=64 ncb=9 nrb=17
    ("complex128", 1024, 1, 302, 32, 216),  # chunks: Rc=1 nchunk=32 CT=128 ncb=8 nrb=64
    ("complex128", 1024, 3, 309, 1, 0),     # chunks: Rc=1 nchunk=1 CT=128 ncb=8 nrb=64
    ("mixed", 1, 1, 0, 1, 0),               # CT=128 ncb=1 nrb=1 Rc=1
    ("mixed", 15, 2, 8, 3, 6),              # CT=128 ncb=1 nrb=1 Rc=1
    ("mixed", 2, 2, 0, 2, 0),               # CT=128 ncb=1 nrb=1 Rc=1
    ("mixed", 16, 1, 7, 3, 3),              # CT=128 ncb=1 nrb=1 Rc=1
    ("mixed", 17, 2, 14, 3, 0),             # CT=64 ncb=1 nrb=1 Rc=1
    ("mixed", 31, 3, 8, 3, 26),             # CT=64 ncb=1 nrb=1 Rc=1
    ("mixed", 18, 1, 9, 3, 1),              # CT=64 ncb=1 nrb=1 Rc=1
    ("mixed", 32, 2, 20, 3, 7),             # CT=64 ncb=1 nrb=1 Rc=1
    ("mixed", 33, 3, 27, 3, 0),             # CT=32 ncb=1 nrb=1 Rc=1
    ("mixed", 63, 1, 2, 3, 46),             # CT=32 ncb=1 nrb=1 Rc=1
    ("mixed", 34, 2, 7, 3, 20),             # CT=32 ncb=1 nrb=1 Rc=1
    ("mixed", 64, 3, 17, 3, 56),            # CT=32 ncb=1 nrb=1 Rc=1
    ("mixed", 65, 1, 21, 65, 0),            # CT=64 ncb=1 nrb=3 Rc=2
    ("mixed", 127, 2, 92, 35, 66),          # CT=64 ncb=1 nrb=4 Rc=2
    ("mixed", 66, 3, 36, 65, 1),            # CT=64 ncb=1 nrb=3 Rc=2
    ("mixed", 128, 1, 106, 33, 76),         # CT=64 ncb=1 nrb=4 Rc=2
    ("mixed", 129, 2, 113, 33, 0),          # CT=128 ncb=1 nrb=9 Rc=2
    ("mixed", 255, 3, 120, 19, 86),         # CT=128 ncb=1 nrb=16 Rc=2
    ("mixed", 130, 1, 127, 33, 91),         # CT=128 ncb=1 nrb=9 Rc=2
    ("mixed", 256, 2, 134, 17, 96),         # CT=128 ncb=1 nrb=16 Rc=2
    ("mixed", 145, 3, 141, 31, 0),          # CT=32 ncb=3 nrb=3 Rc=2
    ("mixed", 959, 1, 148, 3, 106),         # CT=32 ncb=15 nrb=15 Rc=1
    ("mixed", 146, 2, 11, 31, 111),         # CT=32 ncb=3 nrb=3 Rc=2
    ("mixed", 960, 3, 162, 3, 116),         # CT=32 ncb=15 nrb=15 Rc=1
    ("mixed", 321, 1, 169, 15, 0),          # CT=64 ncb=3 nrb=11 Rc=2
    ("mixed", 895, 2, 176, 3, 126),         # CT=64 ncb=7 nrb=28 Rc=1
    ("mixed", 322, 3, 183, 15, 131),        # CT=64 ncb=3 nrb=11 Rc=2
    ("mixed", 896, 1, 190, 3, 136),         # CT=64 ncb=7 nrb=28 Rc=1
    ("mixed", 449, 2, 197, 11, 0),          # CT=128 ncb=2 nrb=29 Rc=2
    ("mixed", 1023, 3, 204, 3, 146),        # CT=128 ncb=4 nrb=64 Rc=1
    ("mixed", 450, 1, 211, 11, 151),        # CT=128 ncb=2 nrb=29 Rc=2
    ("mixed", 1024, 2, 218, 3, 156),        # CT=128 ncb=4 nrb=64 Rc=1
    ("mixed", 64, 1, 43, 64, 0),            # chunks: Rc=1 nchunk=64 CT=32 ncb=1 nrb=1
    ("mixed", 66, 2, 47, 66, 0),            # chunks: Rc=2 nchunk=33 CT=64 ncb=1 nrb=3
    ("mixed", 96, 3, 60, 65, 21),           # chunks: Rc=2 nchunk=33 CT=64 ncb=1 nrb=3
    ("mixed", 158, 1, 96, 157, 0),          # chunks: Rc=6 nchunk=27 CT=32 ncb=3 nrb=3
    ("mixed", 162, 2, 100, 162, 0),         # chunks: Rc=6 nchunk=27 CT=32 ncb=3 nrb=3
    ("mixed", 256, 2, 13, 256, 0),          # chunks: Rc=4 nchunk=64 CT=128 ncb=1 nrb=16
    ("mixed", 322, 1, 274, 322, 0),         # chunks: Rc=3 nchunk=108 CT=64 ncb=3 nrb=11
    ("mixed", 450, 1, 281, 165, 0),         # chunks: Rc=2 nchunk=83 CT=128 ncb=2 nrb=29
    ("mixed", 513, 1, 288, 127, 206),       # chunks: Rc=1 nchunk=127 CT=32 ncb=9 nrb=9
    ("mixed", 1024, 1, 295, 32, 211),       # chunks: Rc=1 nchunk=32 CT=128 ncb=4 nrb=64
    ("mixed", 1024, 2, 302, 1, 216),        # chunks: Rc=1 nchunk=1 CT=128 ncb=4 nrb=64
]
