from .basetrack import TrackState
from .byte_tracker import BYTETracker

__all__ = ('BYTETracker', 'TrackState')
