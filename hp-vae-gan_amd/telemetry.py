"""Per-iteration loss scalars of a train stage without a host synchronisation per iteration.

The reference reads `kl_loss.item()`, `errG.item()` and the rest on every iteration (train_video.py:210-222).  Here the
iteration is replayed as a hipGraph whose outputs are static device tensors that each replay overwrites, so the values are
appended on the device instead: `LossLog.append` launches hpvg_scalar_log_append_f32, which writes one row of a device ring
table [capacity][K] and advances a device cursor.  Captured with the iteration it appends a fresh row on every replay.

`drain()` copies the cursor and the table to the host in ONE device-to-host copy (they share one buffer) and returns the rows
written since the previous drain.  Row counts come from the device cursor only: recording a capture executes nothing and
replays never pass through python, so no host counter could know them.  When more rows than `capacity` were written since
the last drain, the oldest are gone; `drain` returns the newest `capacity` with their true indices and the lost count."""
import numpy as np
import torch

from . import ops
from .lib import LOG_MAX_K


def drain_rows(cursor, last, capacity, table):
    """Host arithmetic of a drain.  cursor: device cursor now; last: cursor at the previous drain; table: host copy of the
    ring [capacity][K].  Returns (indices, rows, lost): the row indices (0-based append counts) still held, oldest first,
    their values [n][K], and how many rows written since `last` were overwritten before this drain."""
    written = cursor - last
    if written < 0:
        raise RuntimeError("loss log: device cursor %d is behind the last drain (%d)" % (cursor, last))
    lost = max(0, written - capacity)
    first = last + lost
    idx = np.arange(first, cursor, dtype=np.int64)
    rows = table[idx % capacity] if len(idx) else np.zeros((0, table.shape[1]), dtype=table.dtype)
    return idx, rows, lost


class LossLog:
    """Device ring of `capacity` rows of `len(columns)` fp32 scalars plus its device cursor (one int32 buffer: cursor, then the
    table's bits)."""

    def __init__(self, columns, capacity=1024, device="cuda"):
        columns = list(columns)
        if not 1 <= len(columns) <= LOG_MAX_K:
            raise ValueError("a loss log holds 1..%d columns, got %d" % (LOG_MAX_K, len(columns)))
        if capacity < 1:
            raise ValueError("capacity must be positive")
        self.columns = columns
        self.capacity = int(capacity)
        K = len(columns)
        self._buf = torch.zeros(1 + self.capacity * K, dtype=torch.int32, device=device)
        self.cursor = self._buf[:1]
        self.table = self._buf[1:].view(torch.float32).view(self.capacity, K)
        self.drained = 0   # device cursor value at the last drain
        self.lost = 0      # rows overwritten before a drain, over the log's life

    def append(self, scalars):
        """Enqueue one row: `scalars` in column order, fp32 device tensors of one element or (tensor, index) pairs."""
        ops.scalar_log_append_(scalars, self.table, self.cursor)

    def drain(self):
        """(indices, rows [n][K] float32, lost) of the rows appended since the previous drain (synchronises the stream)."""
        host = self._buf.cpu().numpy()
        cursor = int(host[0])
        table = host[1:].view(np.float32).reshape(self.capacity, len(self.columns))
        idx, rows, lost = drain_rows(cursor, self.drained, self.capacity, table)
        self.drained = cursor
        self.lost += lost
        return idx, rows.copy(), lost
