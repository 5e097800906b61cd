"""The reference's own flow on the GPU engine: parse an input file in its text format (Models/LPParser.cs), solve it with the
algorithm names of LPSolver (Models/LPSolver.cs:16-76), print the result record.  Needs an MI355X: there is no CPU fallback.
(As in the reference, the revised algorithm fills only the text fields of the record: its numbers are in `Summary` / `Extra`.)

    python examples/quickstart.py [input file]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import linear_programming_solver_lpr381_amd as lpx

path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(__file__), "..", "integration", "Input", "example_input.txt")
problem = lpx.ParseFromText(open(path).read())
solver = lpx.LPSolver()
for name in ("Primal Simplex", "Revised Primal Simplex", "Branch and Bound"):
    res = solver.Solve(problem, name)
    x = None if res.Solution is None else [float(v) for v in res.Solution]
    print(f"{name}: status {res.Status}, z = {res.OptimalValue}, x = {x}")
    print(res.Summary.strip().splitlines()[-1] if res.Summary else "")

# Bounds without rows (not in the reference): the same model with every x_j <= 2 kept beside the tableau by the
# bounded-variable primal simplex; the tableau keeps the shape of the model without the bounds.
res = solver.SolveBounded(problem, upper=2.0)
print(f"Bounded Primal Simplex (x <= 2): status {res.Status}, z = {res.OptimalValue}, x = {[float(v) for v in res.Solution]}, "
      f"at upper bound {[int(v) for v in res.AtUpper]}, events (to zero, to upper, flips) {res.BoundCounts}")

# Many small LPs in ONE launch (not in the reference): one model under three right-hand sides, c, A and the bounds shared.
packed = solver.SolvePacked([3, 5, 2], [[1, 2, 2], [2, 4, 3]], [[10, 15], [11, 15], [9, 14]], upper=[4, 3, 3])
print(f"Packed batch (3 right-hand sides, one launch): status {packed.Status.tolist()}, z = {packed.OptimalValue.tolist()}")

# Branch and bound by bound changes (not in the reference): the integer program 0 <= x_j <= 2 on that one tableau.
res = solver.SolveBnbBounded(problem, upper=2.0)
print(f"Bounded Branch and Bound (x <= 2, integer): status {res.Status}, z = {res.OptimalValue}, x = {[float(v) for v in res.Solution]}, counters {res.BnbInfo}")
