"""A likelihood family lives in csrc/bsc_families.h and nowhere else: the two pass headers name none.

 * csrc/bsc_glm_pass.h and csrc/bsc_predict_pass.h, read as text, hold no comparison of a family id -- the template
   parameters LINK / FAM / FAMILY of old, a struct's GLM_ID / PREDICT_ID, a GLM_* / PREDICT_* / BSC_SCALAR_* constant --
   and name no family struct.  Two lines are allowed, both in csrc/bsc_predict_pass.h and each exactly once:
     - `constexpr bool ORD = ...`: the ordinal family keeps a branch of predict_body of its own;
     - `if constexpr (F::PREDICT_ID == Gamma::PREDICT_ID)`: the Gamma family's fourth predictive slot is written in
       predict_body, because made inside the struct it changes the kernels' instructions (csrc/bsc_families.h).
   The runtime check of the public `link` argument (check_glm_obs_args: its message is pinned by other tests) compares a
   host variable, not a family of the bodies, and is not meant.
 * every family id of include/bayesic_hip.h (BSC_GLM_*, BSC_PREDICT_*, BSC_SCALAR_*) appears in csrc/bsc_families.h.

No device needed."""
import pathlib
import re

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "bayesic_amd" / "csrc"

ID = r"(?:LINK|FAM|FAMILY|[A-Za-z_:]*(?:GLM_ID|PREDICT_ID|SCALAR_ID)|(?:BSC_)?(?:GLM|PREDICT|SCALAR)_[A-Z]+)"
COMPARES = re.compile(r"\b%s\s*[!=]=|[!=]=\s*%s\b" % (ID, ID))
STRUCTS = re.compile(r"\b(?:Logistic|Poisson|Gaussian|NegBin|Gamma|Weibull|Beta|Ordinal)\s*(?:::|\{\}|>)")
ALLOWED = ("constexpr bool ORD = F::PREDICT_ID == PREDICT_ORDINAL;",
           "if constexpr (F::PREDICT_ID == Gamma::PREDICT_ID) {")
HOST_LINK_CHECK = "BSC_REQUIRE(link == BSC_GLM_LOGISTIC || link == BSC_GLM_POISSON,"


def _code(line):
    return line.split("//", 1)[0]


def test_pass_headers_name_no_family():
    seen = []
    for name in ("bsc_glm_pass.h", "bsc_predict_pass.h"):
        for n, line in enumerate((CSRC / name).read_text().splitlines(), 1):
            code = _code(line).strip()
            if not (COMPARES.search(code) or STRUCTS.search(code)):
                continue
            if code == HOST_LINK_CHECK:
                continue
            assert code in ALLOWED and name == "bsc_predict_pass.h", "%s:%d names a family: %s" % (name, n, line)
            seen.append(code)
    assert sorted(seen) == sorted(ALLOWED)


def test_every_public_family_id_is_in_the_family_header():
    public = re.findall(r"^#define (BSC_(?:GLM|PREDICT|SCALAR)_[A-Z]+) \d+$", (ROOT / "include" / "bayesic_hip.h").read_text(),
                        re.M)
    assert set(public) >= {"BSC_GLM_LOGISTIC", "BSC_GLM_POISSON", "BSC_PREDICT_GAUSSIAN", "BSC_PREDICT_LOGISTIC",
                           "BSC_PREDICT_POISSON", "BSC_SCALAR_NEGBIN", "BSC_SCALAR_GAMMA", "BSC_SCALAR_WEIBULL"}
    families = (CSRC / "bsc_families.h").read_text()
    for name in public:
        assert re.search(r"\b%s\b" % name, families), "%s is not in csrc/bsc_families.h" % name
