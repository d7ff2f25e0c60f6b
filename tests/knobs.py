"""The library's experiment knobs (environment variables it reads per call; the table is in mgdt_yolo_amd/csrc/launch_host.h) for the length of a `with`."""
import os
from contextlib import contextmanager


@contextmanager
def knobs(**kv):
    """Set (a string) or unset (None) environment variables for the calls inside; restored afterwards."""
    old = {k: os.environ.get(k) for k in kv}

    def put(values):
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        put(kv)
        yield
    finally:
        put(old)


def forced_tile(tile):
    """MGDT_CSP_TILE='th,tw' for the calls inside; a false `tile` leaves the variable as it is."""
    return knobs(MGDT_CSP_TILE=f'{tile[0]},{tile[1]}') if tile else knobs()
