#!/usr/bin/env python3
"""Record tests/golden/aggregate_expressions_plans.json: what every query of tests/_agg_expr_queries.py lowers to
WITHOUT the ``aggregate_expressions`` opt-in -- its plan string, or the class and message of its error -- under each
set of the other opt-ins the list names.

Run it against the package of the commit BEFORE the opt-in existed (the fixture names that commit), never against the
code under test:

    git archive <commit> giql_amd | tar -x -C <dir>
    PYTHONPATH=<dir> python tests/golden/make_aggregate_expressions_plans.py <commit>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

import _agg_expr_queries as Q  # noqa: E402
from giql_amd.transpile import build_plan  # noqa: E402  (the package on PYTHONPATH)


def main() -> None:
    commit = sys.argv[1]
    assert len(commit) == 40, "name the full commit the package was taken from"
    cases = {name: {opt: Q.outcome(build_plan, query, **kw) for opt, kw in Q.OPTIONS.items()}
             for name, query in Q.ALL.items()}
    with open(os.path.join(HERE, "aggregate_expressions_plans.json"), "w") as f:
        json.dump({"recorded_at_commit": commit, "cases": cases}, f, indent=None, sort_keys=True, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
