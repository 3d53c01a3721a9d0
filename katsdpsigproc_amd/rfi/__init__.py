"""RFI flagging algorithms (reference: src/katsdpsigproc/rfi/__init__.py)."""

import enum

#: ratio of the standard deviation to the median absolute deviation of a normal
#: distribution (reference rfi/__init__.py:31)
MAD_NORMAL = 1.4826


class BackgroundFlags(enum.Enum):
    """How input flags are supplied to a backgrounder (reference rfi/device.py:40-46) or to
    the averager. Lives here so that both :mod:`.host` and :mod:`.device` can name it;
    ``device.BackgroundFlags`` is this class."""

    NONE = 0
    CHANNEL = 1
    FULL = 2

    def __bool__(self) -> bool:
        return self is not BackgroundFlags.NONE
