"""A small timing-ephemeris (.par) reader: the handful of parameters make_fake_pulsar installs
(pplib.py:3265-3296).

It reads PSR or PSRJ, RAJ, DECJ, F0 or P0, PEPOCH and DM, with Fortran 'D' exponents accepted;
every other line is skipped, the `C ...` comment lines included.  There is no predictor here: a
simulated subint's period is 1 / F0 whatever F1 or the binary parameters say.
"""
import numpy as np

_TEXT = ("PSR", "PSRJ", "RAJ", "DECJ")
_NUMBERS = ("F0", "P0", "PEPOCH", "DM")


def _number(tok):
    return np.float64(tok.replace("D", "E").replace("d", "e"))


class psr_par(object):
    """Attributes PSR (PSRJ stands in for it), RAJ, DECJ, F0, P0, PEPOCH, DM of the file `parfile`;
    P0 = 1 / F0 and F0 = 1 / P0 where only one of them is given.  ValueError names what is missing."""

    def __init__(self, parfile):
        self.FILE = str(parfile)
        with open(parfile, "r") as fh:
            lines = fh.readlines()
        for line in lines:
            tok = line.split()
            if len(tok) < 2:
                continue
            key = tok[0]
            if key in _TEXT:
                setattr(self, key, tok[1])
            elif key in _NUMBERS:
                try:
                    setattr(self, key, _number(tok[1]))
                except ValueError:
                    raise ValueError("%s: cannot read %s from %r" % (parfile, key, tok[1]))
        if not hasattr(self, "PSR") and hasattr(self, "PSRJ"):
            self.PSR = self.PSRJ
        if hasattr(self, "F0") and not hasattr(self, "P0"):
            self.P0 = np.float64(1.0) / self.F0
        elif hasattr(self, "P0") and not hasattr(self, "F0"):
            self.F0 = np.float64(1.0) / self.P0
        missing = [k for k in ("PSR", "P0", "PEPOCH", "DM") if not hasattr(self, k)]
        if missing:
            raise ValueError("%s: no %s" % (parfile, ", ".join("F0 or P0" if k == "P0" else
                                                              "PSR or PSRJ" if k == "PSR" else k for k in missing)))
        for k in ("RAJ", "DECJ"):
            if not hasattr(self, k):
                setattr(self, k, None)
