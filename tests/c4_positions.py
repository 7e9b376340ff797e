"""Six placed Connect Four positions shared by tests/test_connect_four_cpu.py and tests/test_gpu_connect_four.py: six columns
full, so exactly one column is legal, and no line of four on the board before the move.  Found once by a random search over
boards with six full columns (a few thousand tries) and pasted here.  (kind, turn, forced column, board[7 * row + col]);
kind names what the forced move does: it completes a line in that one direction only, fills the board without a line
('draw'), or does neither ('plain')."""
import numpy as np

POSITIONS = [
    ('vertical', 1, 3, [-1, 1, 1, 1, -1, -1, -1, -1, -1, -1, 1, -1, 1, 1, -1, 1, 1, 1, -1, 1, 1, 1, -1, -1, 0, 1, 1, -1, 1, 1, -1, 0,
                        -1, -1, 1, 1, 1, 1, 0, 1, 1, 1]),
    ('horizontal', 1, 3, [1, 1, 1, 0, 1, 1, -1, 1, -1, 1, 0, -1, -1, -1, -1, 1, -1, 0, 1, 1, 1, -1, 1, 1, 0, 1, 1, 1, 1, -1, 1, 0,
                          1, -1, -1, 1, 1, 1, 0, -1, 1, 1]),
    ('rising', 1, 4, [1, 1, -1, -1, -1, 1, 1, -1, 1, 1, 1, -1, -1, 1, 1, -1, -1, -1, 0, 1, -1, -1, -1, 1, -1, 0, 1, -1, 1, 1, -1, -1,
                      0, 1, 1, -1, 1, 1, 1, 0, -1, -1]),
    ('falling', -1, 4, [1, -1, 1, -1, 1, -1, 1, 1, 1, 1, -1, 1, 1, -1, -1, 1, -1, 1, -1, -1, -1, -1, 1, -1, -1, 0, 1, 1, -1, -1, 1,
                        -1, 0, 1, 1, 1, 1, 1, -1, 0, -1, -1]),
    ('draw', 1, 3, [-1, -1, -1, 1, -1, -1, -1, -1, 1, 1, -1, 1, 1, -1, -1, -1, 1, 1, 1, -1, 1, 1, 1, -1, -1, 1, -1, 1, -1, -1, -1, 1,
                    -1, -1, -1, 1, -1, 1, 0, -1, 1, 1]),
    ('plain', -1, 2, [-1, 1, 1, -1, -1, 1, -1, -1, 1, 0, 1, -1, 1, -1, -1, 1, 0, -1, 1, 1, 1, 1, -1, 0, 1, 1, -1, -1, -1, -1, 0, 1,
                      1, -1, 1, -1, -1, 0, 1, -1, 1, 1]),
]
POSITIONS = [(k, t, c, np.array(b, np.int32)) for k, t, c, b in POSITIONS]
WINS = ('vertical', 'horizontal', 'rising', 'falling')

# every window of four cells in a line, with its direction: 21 vertical, 24 horizontal, 12 + 12 diagonal
WINDOWS = []
for _r in range(6):
  for _c in range(7):
    for _name, _dr, _dc in (('vertical', 1, 0), ('horizontal', 0, 1), ('rising', 1, 1), ('falling', 1, -1)):
      _cells = [(_r + i * _dr, _c + i * _dc) for i in range(4)]
      if all(0 <= rr < 6 and 0 <= cc < 7 for rr, cc in _cells):
        WINDOWS.append((_name, [7 * rr + cc for rr, cc in _cells]))
assert len(WINDOWS) == 69
_CELLS = np.array([w for _, w in WINDOWS])


def lines_of(board42, player):
  """directions in which `player` has four in a window, scanning all 69 windows of the whole board"""
  hit = np.flatnonzero((np.asarray(board42)[_CELLS] == player).all(1))
  return sorted({WINDOWS[i][0] for i in hit})
