"""reference: tracker/trackers/basetrack.py - the states of a track, as the device table stores them."""


class TrackState:
    New = 0            # in the device table: a free slot
    Tracked = 1
    Lost = 2
    Removed = 3        # a lost track past the buffer, kept in the lost list for one more frame as the reference keeps it (csrc/track.hip)
