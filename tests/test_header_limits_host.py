"""The limits of the measurement entries are read from include/tacotron2_amd.h (_lib.K), not typed again in Python.  The values are
spelled out here, so that changing a limit in the header is a deliberate edit of this file too; the Python attributes that used to
be copies must equal the header's entries; and the parser takes only `#define T2_<NAME> <integer>`."""
from tacotron2_amd import _args, _lib, analysis, engine, loudness, psola, stretch, variance

LIMITS = dict(ALIGN_MAX_L=4096, VAR_MAX_T=4096, VAR_MAX_L=4096, VAR_NSTAT=10, DTW_MAX_T=4096, DTW_MAX_K=32, CEPS_MAX_M=1024,
              YIN_MAX_SPAN=4096, PROSODY_NSTAT=8, PROSODY_MAX_T=4096, VQ_MAX_CYCLES=32, CORPUS_NSTAT=12, PITCH_MAX_STATES=4096,
              F0_NSTAT=12, STRETCH_MAX_N=2048, STRETCH_MAX_D=1024, PSOLA_MIN_LAG=16, PSOLA_MAX_LAG=4096, PSOLA_MIN_RHO=16384,
              PSOLA_MAX_RHO=262144, PSOLA_SYN_TAIL=10256, LOUD_NSTAT=10, LOUD_MAX_K=4096)
STATUS = ("OK", "ERR_ARG", "ERR_LAUNCH", "ERR_RESIDENCY")


def test_the_header_holds_these_limits_and_no_others():
    assert {k: v for k, v in _lib.K.items() if k not in STATUS} == LIMITS
    assert all(type(v) is int for v in _lib.K.values())


def test_python_attributes_are_the_header_entries():
    K = _lib.K
    pairs = [(analysis.PROSODY_MAX_T, "PROSODY_MAX_T"), (analysis.PROSODY_NSTAT, "PROSODY_NSTAT"), (analysis.VQ_MAX_CYCLES, "VQ_MAX_CYCLES"),
             (analysis.CORPUS_NSTAT, "CORPUS_NSTAT"), (analysis.PITCH_MAX_STATES, "PITCH_MAX_STATES"), (analysis.F0_NSTAT, "F0_NSTAT"),
             (_args.YIN_MAX_SPAN, "YIN_MAX_SPAN"), (analysis.YIN_MAX_SPAN, "YIN_MAX_SPAN"),
             (variance.VAR_MAX_T, "VAR_MAX_T"), (variance.VAR_MAX_L, "VAR_MAX_L"), (variance.VAR_NSTAT, "VAR_NSTAT"),
             (stretch.MAX_FRAME, "STRETCH_MAX_N"), (stretch.MAX_TOLERANCE, "STRETCH_MAX_D"),
             (psola.LAG_RANGE[0], "PSOLA_MIN_LAG"), (psola.LAG_RANGE[1], "PSOLA_MAX_LAG"), (psola.RHO_RANGE[0], "PSOLA_MIN_RHO"),
             (psola.RHO_RANGE[1], "PSOLA_MAX_RHO"), (psola.SYN_TAIL, "PSOLA_SYN_TAIL"), (loudness.NSTAT, "LOUD_NSTAT"),
             (engine.Engine.ALIGN_MAX_L, "ALIGN_MAX_L"), (engine.Engine.DTW_MAX_T, "DTW_MAX_T"), (engine.Engine.DTW_MAX_K, "DTW_MAX_K")]
    for got, name in pairs:
        assert got == K[name], name
    assert len(psola.LAG_RANGE) == 2 and len(psola.RHO_RANGE) == 2


def test_only_integer_defines_outside_comments_are_taken(tmp_path):
    h = tmp_path / "h.h"
    h.write_text("#define T2_A 7\n"
                 "  #  define T2_B 0x10   /* hex, and a comment behind it */\n"
                 "#define T2_NEG -3\n"
                 "/* #define T2_IN_BLOCK 1\n"
                 "#define T2_IN_BLOCK_TOO 2 */\n"
                 "// #define T2_IN_LINE 3\n"
                 "#define T2_FLOAT 1.5\n"
                 "#define T2_EXPR (1 << 4)\n"
                 "#define T2_SUFFIX 4096u\n"
                 "#define T2_NAME T2_A\n"
                 "#define T2_EMPTY\n"
                 "#define T2_FN(x) 3\n"
                 "#define OTHER_C 9\n"
                 "int x = 5; #define T2_MIDLINE 5\n")
    assert _lib._parse_header(str(h))[3] == {"A": 7, "B": 16, "NEG": -3}
