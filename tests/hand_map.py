"""The 5x5 map small enough to work out by hand that the policy-field, sampled-field and pose-field tests share."""
# a corridor of three cells, (1, 1) (2, 1) (3, 1), the last one the goal; everything else is wall
HAND_WALLS = [31, 17, 31, 31, 31]
HAND_GOAL = (3, 1)
# (x, y, dir): action -- written down with its consequence
HAND_ACTIONS = {
    (2, 1, 0): 2,  # forward into the goal: steps 1, dist 1
    (2, 1, 1): 0,  # left to (2,1,0): steps 2, dist 2, optimal
    (2, 1, 2): 0,  # left to (2,1,1): steps 3, dist 3, optimal
    (2, 1, 3): 0,  # left to (2,1,2): steps 4, dist 2 (right would face the goal), not optimal
    (1, 1, 0): 2,  # forward to (2,1,0): steps 2, dist 2, optimal
    (1, 1, 1): 1,  # right to (1,1,2): trapped, dist 3
    (1, 1, 2): 2,  # forward into the wall at (0,1): trapped, dist 4
    (1, 1, 3): 1,  # right to (1,1,0): steps 3, dist 3, optimal
    (3, 1, 2): 2,  # forward to (2,1,2): steps 4, dist 4, optimal
    (3, 1, 1): 1,  # right to (3,1,2): steps 5, dist 5, optimal
    (3, 1, 3): 1,  # right to (3,1,0): steps 7, dist 5: beyond max_steps 5, not optimal
    (3, 1, 0): 1,  # right to (3,1,1): steps 6, dist 6: not solvable within 5
}
HAND_STEPS = {(2, 1, 0): 1, (2, 1, 1): 2, (2, 1, 2): 3, (2, 1, 3): 4, (1, 1, 0): 2, (1, 1, 1): -1, (1, 1, 2): -1,
              (1, 1, 3): 3, (3, 1, 2): 4, (3, 1, 1): 5, (3, 1, 3): 7, (3, 1, 0): 6}
HAND_DIST = {(2, 1, 0): 1, (2, 1, 1): 2, (2, 1, 2): 3, (2, 1, 3): 2, (1, 1, 0): 2, (1, 1, 1): 3, (1, 1, 2): 4,
             (1, 1, 3): 3, (3, 1, 2): 4, (3, 1, 1): 5, (3, 1, 3): 5, (3, 1, 0): 6}
