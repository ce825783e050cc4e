"""The preparation of a low-resolution depth map between the file and the upsample: which steps run -- hole
filling (12.9), guided (12.11) or not, and per-image range normalisation (12.10) -- is ONE record, LrPrep.  Its fields are the
keyword arguments of infer.run_loop, train.TrainSet and train.fit, the keys of a `val` dict and of a checkpoint's args; its
checks, its chain of launches and its command-line flags are stated here once."""
import dataclasses

from .upsample import FILL_SIGMA, check_fill_sigma, check_stretch_top, fill_holes, fill_holes_guided, stretch_codes


@dataclasses.dataclass(frozen=True)
class LrPrep:
    fill_holes: bool = False        # fill the holes by pull-push (upsample.fill_holes)
    fill_guided: bool = False       # ... with the guidance's say (upsample.fill_holes_guided); needs fill_holes
    fill_sigma: float = FILL_SIGMA  # ... under the range table of this sigma, in guidance codes; the default without fill_guided
    normalize: bool = False         # then stretch the map's own range onto the code grid (upsample.stretch_codes)

    def __post_init__(self):
        for name in ("fill_holes", "fill_guided", "normalize"):
            object.__setattr__(self, name, bool(getattr(self, name)))
        object.__setattr__(self, "fill_sigma", float(self.fill_sigma) if self.fill_guided else FILL_SIGMA)

    @classmethod
    def checked(cls, who: str, fill_holes=False, fill_guided=False, fill_sigma=FILL_SIGMA, normalize=False, *, lr=None,
                top: int = None, normalize_needs_lr: bool = True) -> "LrPrep":
        """The record of caller `who`'s keyword arguments, refused by name where they do not go together.  lr: (the name of the
        caller's low-resolution argument, whether it was given) -- fill_holes, and normalize unless the caller stretches other
        planes too, need it, and fill_guided needs fill_holes; None for a caller with rules of its own about where the options
        apply (fit).  top: the code of 1.0, checked for normalize."""
        if lr is not None:
            name, given = lr
            if fill_holes and not given:
                raise ValueError(f"{who}: fill_holes needs {name} (only low-resolution code planes are filled)")
            if fill_guided and not fill_holes:
                raise ValueError(f"{who}: fill_guided needs fill_holes (it chooses how the holes are filled)")
        if fill_guided:
            fill_sigma = check_fill_sigma(who, fill_sigma)
        if lr is not None and normalize and normalize_needs_lr and not lr[1]:
            raise ValueError(f"{who}: normalize needs {lr[0]} (input_depth maps are not code planes: only low-resolution codes "
                             "are normalised)")
        if normalize and top is not None:
            check_stretch_top(f"{who}: normalize", top)
        return cls(fill_holes, fill_guided, fill_sigma, normalize)

    @classmethod
    def from_mapping(cls, m) -> "LrPrep":
        """The record of a `val` dict, a checkpoint's args or vars(namespace): a missing key, or None, is the field's default."""
        return cls(**{f.name: m[f.name] for f in dataclasses.fields(cls) if m.get(f.name) is not None})

    @classmethod
    def defaults(cls, *names) -> dict:
        return {f.name: f.default for f in dataclasses.fields(cls) if f.name in names}

    def set_options(self) -> dict:
        """The options that are set, and nothing else: what a caller passes on as keyword arguments, what a `val` dict holds
        and what a checkpoint's args gain -- a run without an option keeps exactly the keys it always had."""
        return {**({"fill_holes": True} if self.fill_holes else {}),
                **({"fill_guided": True, "fill_sigma": self.fill_sigma} if self.fill_guided else {}),
                **({"normalize": True} if self.normalize else {})}

    def fill(self, codes, guide, scale: int, depth_max):
        """codes, filled as the record says; guide is read with fill_guided only"""
        if self.fill_guided:
            return fill_holes_guided(codes, guide, scale, self.fill_sigma, depth_max)
        return fill_holes(codes, depth_max) if self.fill_holes else codes

    def apply(self, codes, guide, scale: int, depth_max):
        """(codes', lo_hi): [fill ->] [stretch] of a plane of codes on the device; lo_hi is stretch_codes' range, for
        unstretch_codes, or None without normalize.  depth_max: None for 8-bit codes, as the upsample functions take it."""
        codes = self.fill(codes, guide, scale, depth_max)
        return stretch_codes(codes, depth_max) if self.normalize else (codes, None)


def add_prep_args(ap, help: dict):
    """The record's flags; every command line words its own help ({"fill_holes": ..., ...})."""
    ap.add_argument("--fill-holes", action="store_true", help=help["fill_holes"])
    ap.add_argument("--fill-guided", action="store_true", help=help["fill_guided"])
    ap.add_argument("--fill-sigma", type=float, default=None, metavar="CODES",
                    help=f"with --fill-guided: the sigma of the range weight in guidance codes (default {FILL_SIGMA}, untuned)")
    ap.add_argument("--normalize", action="store_true", help=help["normalize"])


def prep_of(ap, a, guided_ok: bool, guided_needs: str) -> LrPrep:
    """The record of the parsed flags, a.fill_sigma resolved to its default; the refusals every command line shares go through
    ap.error (where the other flags apply is the command line's own business, and is refused there)."""
    if a.fill_guided and not guided_ok:
        ap.error(f"--fill-guided needs {guided_needs}")
    if a.fill_sigma is not None and not a.fill_guided:
        ap.error("--fill-sigma needs --fill-guided")
    if a.fill_sigma is not None and not (0.0 < a.fill_sigma < float("inf")):
        ap.error(f"--fill-sigma {a.fill_sigma} must be positive")
    a.fill_sigma = FILL_SIGMA if a.fill_sigma is None else float(a.fill_sigma)
    return LrPrep(a.fill_holes, a.fill_guided, a.fill_sigma, a.normalize)
