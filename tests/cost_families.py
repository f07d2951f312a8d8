"""The cost families of the test suite, listed once: every truth module, in the order the families were added.  A truth module
describes its pairs (PAIRS, PARAMS, grid, truth, host_cost, gpu_cost, ...) and, next to them, what the shared batteries need of
the family as data (train_y, train_costs, CHECKPOINT, check_trained_cost, check_elements, VALUE_TRUTH_FINITE, and for the route
battery ROUTE_PAIR, ROUTE_RUNTIME_PAIR and ROUTE_SMALL_RANK_SETS).  tests/step_fixtures.py, tests/test_gpu_cost_routes.py and
the tests/test_gpu_family_cost_{train,elements,routes}.py batteries reach a family through this module alone: a new family
appends its truth module to TRUTH_MODULES.  (tests/test_gpu_{beta,gamma}_cost_routes.py hold the route tests of those two
families and take the three ROUTE_ names from the truth module as well; the route battery runs every other family.)

Importing this module imports every truth module (the pair table below is built and checked once, here), and
tests/step_fixtures.py imports this module: a truth module that needs step_fixtures imports it inside the function that uses it."""
import beta_cost_truth
import cost_truth
import count_cost_truth
import gamma_cost_truth
import ordinal_cost_truth

TRUTH_MODULES = [cost_truth, count_cost_truth, beta_cost_truth, ordinal_cost_truth, gamma_cost_truth]
FAMILIES = TRUTH_MODULES[1:]  # every module but the reference's pairs: the families with instantiations of their own

_owner = {}
for _module in TRUTH_MODULES:
    for _pair in _module.PAIRS:
        assert _pair not in _owner, f"{_pair} occurs in {_owner[_pair].__name__} and in {_module.__name__}"
        _owner[_pair] = _module
for _module in FAMILIES:  # family_cells() builds a selector problem for the sets "a" and "b" of every family
    assert {"a", "b"} <= set(_module.PARAMS), f"{_module.__name__} must state the parameter sets a and b"
    assert _module.ROUTE_PAIR in _module.PAIRS, f"{_module.__name__} does not describe its route pair {_module.ROUTE_PAIR}"
    assert _module.ROUTE_RUNTIME_PAIR is None or _module.ROUTE_RUNTIME_PAIR in _module.PAIRS, (
        f"{_module.__name__} does not describe its run-time route pair {_module.ROUTE_RUNTIME_PAIR}")


def truth_module(pair):
    """The truth module that describes the pair's family (a pair name occurs in one of them only): its grid, mpmath truth,
    recorded errors and bound, host and library cost, and what the selector problems take from it (SELECTOR_RANGE,
    OWN_CARRIER_STREAM, MODES_AGREE)."""
    if pair not in _owner:
        raise KeyError(f"no truth module describes the pair {pair}")
    return _owner[pair]


def family_name(module):
    """count, beta, ordinal, gamma: the family's name in test ids and file names"""
    return module.__name__[: -len("_cost_truth")]


def family_cells():
    """(pair, parameter set) of every family's pairs with the two parameter sets each of them states, "a" and "b": the cells a
    selector problem is built for"""
    return [(pair, pset) for module in FAMILIES for pair in module.PAIRS for pset in "ab"]
