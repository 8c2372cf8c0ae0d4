"""``ConstraintCollocator`` / ``Problem`` with the reference's API surface
(``opty/direct_collocation.py:93-145``, ``:1379-1411``) and one backend:
``'hip'`` -- hand-scheduled gfx950 kernels generated per problem by
:mod:`opty_amd.codegen` and run through ``libopty_hip.so``.

The host-side transcription (symbol classification, discrete symbols,
discretisation, argument / ``wrt`` ordering, instance-constraint index map)
follows the reference's rules so that ``constraints(free)``,
``jacobian(free)`` and ``jacobian_indices()`` have identical layouts:

* unknown parameters / trajectories are name-sorted, known ones keep the
  order of the user's dictionaries (``opty/direct_collocation.py:1940-1950``);
* backward Euler: ``x' -> (x_i - x_p)/h``; midpoint: ``x' -> (x_n - x_i)/h``,
  ``x -> (x_i + x_n)/2`` (``:2143-2156``);
* ``wrt`` = ``x_i, x_p|x_n, u_i[, u_n], p_unknown[, h]`` (``:2719-2737``).
"""

import logging
import os

import numpy as np
import sympy as sm
import sympy.physics.mechanics as me

from .utils import parse_free, sort_sympy
from .codegen.program import build_program, build_hessian_program, \
    build_jacobian_product_program, \
    varying_copies
from .codegen.emit_hip import emit_module, EmitOptions
from . import build_ladder as bl
from . import hip_backend as hb
from . import isa_check
from .marshal import on_device, column_major, check_vector, host_vector, \
    host_vectors, host_block, device_vector, device_vectors, device_block, \
    wait_for_torch, call_vectors, call_block, tensor_operands

__all__ = ['Problem', 'ConstraintCollocator', 'ShardedProblem']

logger = logging.getLogger(__name__)

_METHODS = ('backward euler', 'midpoint')


class ConstraintCollocator(object):
    """Generates the constraint function and the sparse Jacobian of the
    constraint function of a direct-collocation transcription, evaluated on an
    MI355X.

    Same constructor arguments, attributes and public methods as the
    reference's class (``opty/direct_collocation.py:1406-1411``,
    ``:1556-1892``, ``:2450``, ``:3003-3015``).  Differences:

    * ``backend`` must be ``'hip'`` (default); the reference's CPU backends
      ``'cython'`` / ``'numpy'`` do not exist here;
    * ``parallel`` is accepted and ignored (a GPU launch is always parallel);
    * ``tmp_dir`` is the code-object cache directory;
    * extra keywords ``device`` (HIP ordinal), ``emit_options``,
      ``launch_nodes`` (constraint nodes per launch when the handle evaluates
      node shards, :mod:`opty_amd.sharded`) and
      ``jacobian_layout='csr'``: opt-in, stores the Jacobian values sorted by
      row then column (see ``jacobian_csr_structure``);
      ``jacobian_layout='varying_first'``: opt-in, for solvers on the host:
      the same triplets as the reference's, ordered ``[entries that can
      change, all nodes | entries that repeat one of those | node-invariant
      entries | instance partials]`` (IPOPT takes triplets in any order,
      ``opty/direct_collocation.py:527-562``), so that ``jacobian(free)``
      is one PCIe stream into the head of the persistent array -- no host
      scatter (see ``jacobian_segments``);
      ``prune_zeros``: opt-in, drops the structurally zero entries of the
      per-node block from ``jacobian(free)`` / ``jacobian_indices()`` (the
      reference keeps them, ``opty/direct_collocation.py:2589-2593``; 61 % of
      the 10-link pendulum's block) -- SURVEY.md 8(f) rank 3.

    Notation: N nodes, M equations, n states, m input trajectories, q unknown
    input trajectories, r unknown parameters, s variable duration, o instance
    constraints.
    """

    def __init__(self, equations_of_motion, state_symbols,
                 num_collocation_nodes, node_time_interval,
                 known_parameter_map={}, known_trajectory_map={},
                 instance_constraints=None, time_symbol=None, tmp_dir=None,
                 integration_method='backward euler', parallel=False,
                 show_compile_output=False, backend='hip', device=0,
                 emit_options=None, prune_zeros=False,
                 jacobian_layout='coo', launch_nodes=None,
                 deterministic=False, verify_builds=None,
                 specialize_parameters=None):
        # True: the node-invariant sub-expressions (products of masses and
        # lengths, 1/h ...) are printed into the kernels as float64 literals,
        # computed on the host from the known parameter values and the fixed
        # node time interval at build time, instead of being read from the
        # table opty_uni fills: no scalar loads, no scalar registers spilled
        # into vector lanes in the waves at the register limit (the
        # muscle-driven leg: -11 %).  The module is then specific to those
        # values: when known_parameter_map changes between calls (it is
        # re-read on every call, as in the reference) the kernels are printed
        # and compiled again -- seconds, not microseconds: for solves with
        # fixed parameters.
        # None (the default since r06) = automatic: the generic module is
        # built first; when its fused kernel spills at least
        # ``_AUTO_SPECIALIZE_SGPR_SPILLS`` scalar registers into vector lanes
        # -- the class that gains (the muscle-driven leg: 255-377 spilled
        # SGPRs, -7 ... -13 %; not the biped, 58 spilled, which is no faster;
        # not the 24-link stand-ins, store-bound blocks of 5 100 entries that
        # would gain 3 % for a second compile of minutes) -- and there are
        # known parameters to print,
        # the specialised module takes its place.  A caller whose known
        # parameters keep changing (two rebuilds) is moved back to the
        # generic module for good.  False: never.
        if specialize_parameters not in (None, True, False):
            raise ValueError('specialize_parameters must be None, True or '
                             'False.')
        self._specialize_mode = specialize_parameters
        self._specialize = specialize_parameters is True
        self._auto_specialized = False
        self._respecializations = 0
        self._specialized_for = None
        self._literal_values = None
        # how builds are held to the expression DAG before their first use
        # (:meth:`_verify_build`): None = the environment (OPTY_CROSS_CHECK)
        # or every build; 'all', 'hot' (only kernels at the register limit)
        # or 'off'
        if verify_builds not in (None, 'all', 'hot', 'off'):
            raise ValueError("verify_builds must be None, 'all', 'hot' or "
                             "'off'.")
        self._verify_mode = verify_builds
        # opt-in: values that do not depend on the launch a node is evaluated
        # in (node window, shard, strip count, fused or separate kernels) --
        # bit for bit, as the reference's are (one scalar function per node,
        # opty/utils.py:483-494).  The kernels are built without FMA
        # contraction and with one fixed form of every sin / cos pair
        # (``EmitOptions.deterministic``), so that every entry is the same
        # sequence of individually rounded operations whichever wave
        # evaluates it.
        self._deterministic = bool(deterministic)
        self._prune_zeros = bool(prune_zeros)
        # constraint nodes one launch covers (a node shard evaluates fewer
        # than N - 1): picks the kernels' strip count for small launches
        self._launch_nodes = launch_nodes
        if jacobian_layout not in ('coo', 'csr', 'varying_first'):
            raise ValueError('jacobian_layout must be "coo", "csr" or '
                             '"varying_first".')
        if jacobian_layout == 'varying_first' and prune_zeros:
            raise ValueError("jacobian_layout='varying_first' keeps the "
                             "reference's dense block: not with prune_zeros.")
        self._jacobian_layout = jacobian_layout
        self._eom = sm.ImmutableDenseMatrix(equations_of_motion)
        if self._eom.shape[1] != 1:
            raise ValueError('equations_of_motion must be a column matrix.')
        if time_symbol is not None:
            self._time_symbol = time_symbol
            # the reference also re-points mechanics' global time symbol
            # (opty/direct_collocation.py:1490-1494)
            me.dynamicsymbols._t = time_symbol
        else:
            self._time_symbol = me.dynamicsymbols._t

        self._state_symbols = tuple(state_symbols)
        if len(self.state_symbols) != len(set(self.state_symbols)):
            raise ValueError('State symbols must be unique.')
        if backend != 'hip':
            raise ValueError('backend must be "hip" (this build has no '
                             '"cython"/"numpy" CPU backends).')
        self._state_derivative_symbols = tuple(
            s.diff(self.time_symbol) for s in self.state_symbols)
        self._num_collocation_nodes = int(num_collocation_nodes)

        if isinstance(node_time_interval, sm.Symbol):
            self._time_interval_symbol = node_time_interval
            self._variable_duration = True
        else:
            self._time_interval_symbol = sm.Symbol('h_opty', real=True)
            self._variable_duration = False
        self._node_time_interval = node_time_interval

        self._known_parameter_map = known_parameter_map
        self._known_trajectory_map = known_trajectory_map
        self._instance_constraints = instance_constraints
        self._num_constraints = self.num_eom*(self.num_collocation_nodes - 1)
        self._tmp_dir = tmp_dir
        self._parallel = parallel
        self._show_compile_output = show_compile_output
        self._backend = backend
        self._device = int(device)
        # printer options: the caller's, else (generate_source) the measured
        # launch plan of this problem and launch size, else the printer's own
        # rules
        self._emit_options = emit_options
        self._pinned = None         # (EmitOptions, hipcc switches), see
        #                             _verified_alternative
        self._built_options = None
        # why the run form of the restricted kernels (EmitOptions.var_order)
        # failed a build gate: the module's dispatch form then serves
        self._run_form_refused = None
        self._tape = None           # instruction tape of the program's DAG

        self._sort_parameters()
        self._sort_trajectories()
        self._num_free = ((self.num_states +
                           self.num_unknown_input_trajectories) *
                          self.num_collocation_nodes +
                          self.num_unknown_parameters +
                          int(self._variable_duration))
        self._check_known_trajectories()

        if integration_method not in _METHODS:
            raise ValueError('{} is not a valid integration method.'
                             .format(integration_method))
        self._integration_method = integration_method
        self._discrete_symbols()
        self._discretize_eom()

        if instance_constraints is not None:
            self._num_instance_constraints = len(instance_constraints)
            self._num_constraints += self.num_instance_constraints
            self._identify_functions_in_instance_constraints()
            self._find_closest_free_index()
            self._order_instance_atoms()
        else:
            self._num_instance_constraints = 0
            self._inst_atoms = []
            self._inst_rows = np.zeros(0, dtype=np.int64)
            self._inst_cols = np.zeros(0, dtype=np.int64)

        self._program = None
        self._hip = None

    # ------------------------------------------------------------------
    # public attributes (names as in opty/direct_collocation.py:1556-1892)
    # ------------------------------------------------------------------
    eom = property(lambda self: self._eom)
    time_symbol = property(lambda self: self._time_symbol)
    state_symbols = property(lambda self: self._state_symbols)
    state_derivative_symbols = property(
        lambda self: self._state_derivative_symbols)
    num_collocation_nodes = property(
        lambda self: self._num_collocation_nodes)
    node_time_interval = property(lambda self: self._node_time_interval)
    time_interval_symbol = property(lambda self: self._time_interval_symbol)
    known_parameter_map = property(lambda self: self._known_parameter_map)
    known_trajectory_map = property(lambda self: self._known_trajectory_map)
    instance_constraints = property(lambda self: self._instance_constraints)
    num_constraints = property(lambda self: self._num_constraints)
    num_free = property(lambda self: self._num_free)
    num_instance_constraints = property(
        lambda self: self._num_instance_constraints)
    tmp_dir = property(lambda self: self._tmp_dir)
    parallel = property(lambda self: self._parallel)
    show_compile_output = property(lambda self: self._show_compile_output)
    discrete_eom = property(lambda self: self._discrete_eom)
    known_parameters = property(lambda self: self._known_parameters)
    num_known_parameters = property(lambda self: len(self._known_parameters))
    unknown_parameters = property(lambda self: self._unknown_parameters)
    num_unknown_parameters = property(
        lambda self: len(self._unknown_parameters))
    parameters = property(lambda self: self._parameters)
    num_parameters = property(lambda self: len(self._parameters))
    known_input_trajectories = property(
        lambda self: self._known_input_trajectories)
    num_known_input_trajectories = property(
        lambda self: len(self._known_input_trajectories))
    unknown_input_trajectories = property(
        lambda self: self._unknown_input_trajectories)
    num_unknown_input_trajectories = property(
        lambda self: len(self._unknown_input_trajectories))
    input_trajectories = property(lambda self: self._input_trajectories)
    num_input_trajectories = property(
        lambda self: len(self._input_trajectories))
    previous_discrete_state_symbols = property(
        lambda self: self._previous_discrete_state_symbols)
    current_discrete_state_symbols = property(
        lambda self: self._current_discrete_state_symbols)
    next_discrete_state_symbols = property(
        lambda self: self._next_discrete_state_symbols)
    current_known_discrete_specified_symbols = property(
        lambda self: self._current_known_discrete_specified_symbols)
    next_known_discrete_specified_symbols = property(
        lambda self: self._next_known_discrete_specified_symbols)
    current_unknown_discrete_specified_symbols = property(
        lambda self: self._current_unknown_discrete_specified_symbols)
    next_unknown_discrete_specified_symbols = property(
        lambda self: self._next_unknown_discrete_specified_symbols)
    current_discrete_specified_symbols = property(
        lambda self: self._current_discrete_specified_symbols)
    next_discrete_specified_symbols = property(
        lambda self: self._next_discrete_specified_symbols)

    @property
    def num_eom(self):
        return self._eom.shape[0]

    @property
    def num_states(self):
        return len(self._state_symbols)

    @property
    def integration_method(self):
        return self._integration_method

    @integration_method.setter
    def integration_method(self, method):
        if method not in _METHODS:
            raise ValueError('{} is not a valid integration method.'
                             .format(method))
        self._integration_method = method
        self._discretize_eom()
        self._program = None
        self._hip = None

    @property
    def num_block_columns(self):
        """C: columns of the per-node dense block (``len(wrt)``)."""
        q = self.num_unknown_input_trajectories
        return (2*self.num_states +
                (q if self.integration_method == 'backward euler' else 2*q) +
                self.num_unknown_parameters + int(self._variable_duration))

    # ------------------------------------------------------------------
    # symbol classification (opty/direct_collocation.py:1904-2035)
    # ------------------------------------------------------------------
    @staticmethod
    def _parse_inputs(all_syms, known_syms):
        """-> (known, unknown): known in the user's order, unknown sorted."""
        pool = set(all_syms)
        known_syms = list(known_syms)
        if not pool:
            if known_syms:
                raise ValueError('{} are not in the provided equations of '
                                 'motion.'.format(known_syms))
            return (), ()
        known = tuple(known_syms)
        return known, tuple(sort_sympy(pool.difference(known)))

    def _sort_parameters(self):
        pool = set(self.eom.free_symbols)
        pool.discard(self.time_symbol)
        known, unknown = self._parse_inputs(pool,
                                            self.known_parameter_map.keys())
        self._known_parameters = known
        self._unknown_parameters = unknown
        self._parameters = known + unknown

    def _sort_trajectories(self):
        state_related = set(self.state_symbols).union(
            self.state_derivative_symbols)
        non_states = me.find_dynamicsymbols(self.eom).difference(
            state_related)
        if any(isinstance(f, sm.Derivative) for f in non_states):
            raise ValueError('Too few state variables provided for state '
                             'time derivatives found in equations of motion.')
        # non-state functions may be explicit functions of time, r(t), or
        # implicit ones through a single state, r(x(t)); the latter need the
        # user to supply dr/dx as a known trajectory as well
        # (opty/direct_collocation.py:2009-2018)
        self._deriv_in_knw_traj = False
        for f in non_states:
            if len(f.args) > 1:
                raise ValueError(f'{f} is a function of more than one '
                                 'variable.')
            if f.args != (self.time_symbol,):
                if f.args[0] not in self.state_symbols:
                    raise ValueError(f'{f} must be a function of time or of '
                                     'one state.')
                self._deriv_in_knw_traj = True
        names = [f.name for f in non_states]
        if len(names) != len(set(names)):
            raise ValueError('Repeated input trajectory variable fnames not '
                             f'allowed: {names}')
        known, unknown = self._parse_inputs(non_states,
                                            self.known_trajectory_map.keys())
        self._known_input_trajectories = known
        self._unknown_input_trajectories = unknown
        self._input_trajectories = known + unknown

    def _check_known_trajectories(self):
        N = self.num_collocation_nodes
        for k, v in self.known_trajectory_map.items():
            if callable(v):
                v = v(np.ones(self.num_free))
            if len(v) != N:
                raise ValueError('The known parameter {} is not length {}.'
                                 .format(k, N))

    # ------------------------------------------------------------------
    # discretisation (opty/direct_collocation.py:2037-2156)
    # ------------------------------------------------------------------
    def _discrete_symbols(self):
        def tagged(funcs, tag):
            return tuple(sm.Symbol(f.__class__.__name__ + tag, real=True)
                         for f in funcs)
        self._previous_discrete_state_symbols = tagged(self.state_symbols,
                                                       'p')
        self._current_discrete_state_symbols = tagged(self.state_symbols, 'i')
        self._next_discrete_state_symbols = tagged(self.state_symbols, 'n')
        def known(f, tag):
            # (opty/direct_collocation.py:2080-2093)
            if isinstance(f, sm.Derivative):          # dr(x(t))/dx(t)
                var, (wrt, _) = f.args
                return sm.Symbol('d' + var.__class__.__name__ + tag + '_d' +
                                 wrt.__class__.__name__ + tag, real=True)
            if f.args[0] != self.time_symbol:         # r(x(t))
                arg = sm.Symbol(f.args[0].__class__.__name__ + tag,
                                real=True)
                return sm.Function(f.__class__.__name__ + tag,
                                   real=True)(arg)
            return sm.Symbol(f.__class__.__name__ + tag, real=True)

        self._current_known_discrete_specified_symbols = tuple(
            known(f, 'i') for f in self.known_input_trajectories)
        self._next_known_discrete_specified_symbols = tuple(
            known(f, 'n') for f in self.known_input_trajectories)
        self._current_unknown_discrete_specified_symbols = tagged(
            self.unknown_input_trajectories, 'i')
        self._next_unknown_discrete_specified_symbols = tagged(
            self.unknown_input_trajectories, 'n')
        self._current_discrete_specified_symbols = (
            self._current_known_discrete_specified_symbols +
            self._current_unknown_discrete_specified_symbols)
        self._next_discrete_specified_symbols = (
            self._next_known_discrete_specified_symbols +
            self._next_unknown_discrete_specified_symbols)

    def _create_function_replacements(self):
        """``{r_i(x_i): Symbol('rixi'), d r_i(x_i)/d x_i: Symbol('dri_dxi')}``
        for every implicit known trajectory, current and next
        (``opty/direct_collocation.py:2284-2302``).  The HIP backend does not
        substitute: it lowers ``r_i(x_i)`` as an input row whose derivative
        with respect to ``x_i`` is the row of ``dri_dxi`` (see
        ``_implicit_chain``); this method exists for API parity."""
        repl = {}
        for f in (self.current_known_discrete_specified_symbols +
                  self.next_known_discrete_specified_symbols):
            if isinstance(f, sm.Function) and \
                    f.args[0] != self.time_symbol:
                repl[f.diff()] = sm.Symbol(
                    'd' + f.__class__.__name__ + '_d' + str(f.args[0]),
                    real=True)
                repl[f] = sm.Symbol(f.__class__.__name__ + str(f.args[0]),
                                    real=True)
        return repl

    def _implicit_chain(self):
        """``[(index of r in input_trajectories, state index of its argument,
        index of dr/dx in input_trajectories)]``."""
        links = []
        traj = self.input_trajectories
        for k, f in enumerate(traj):
            if isinstance(f, sm.Derivative) or \
                    f.args == (self.time_symbol,):
                continue
            arg = f.args[0]
            deriv = sm.Derivative(f, arg)
            if deriv not in traj:
                raise ValueError(
                    f'{f} is a function of the state {arg}: its derivative '
                    f'{deriv} must be supplied in known_trajectory_map.')
            links.append((k, self.state_symbols.index(arg),
                          traj.index(deriv)))
        return links

    def _discretize_eom(self):
        logger.info('Discretizing the equations of motion.')
        x, xd = self.state_symbols, self.state_derivative_symbols
        u = self.input_trajectories
        xp = self.previous_discrete_state_symbols
        xi = self.current_discrete_state_symbols
        xn = self.next_discrete_state_symbols
        ui = self.current_discrete_specified_symbols
        un = self.next_discrete_specified_symbols
        h = self.time_interval_symbol
        rules = {}
        if self.integration_method == 'backward euler':
            for d, cur, prev in zip(xd, xi, xp):
                rules[d] = (cur - prev)/h
            rules.update(zip(x + u, xi + ui))
        else:
            for d, cur, nxt in zip(xd, xi, xn):
                rules[d] = (nxt - cur)/h
            for f, cur, nxt in zip(x + u, xi + ui, xn + un):
                rules[f] = (cur + nxt)/2
        # one top-down pass: derivatives are matched before their arguments
        self._discrete_eom = self.eom.xreplace(rules)

    # ------------------------------------------------------------------
    # instance constraints (opty/direct_collocation.py:2158-2282)
    # ------------------------------------------------------------------
    def _identify_functions_in_instance_constraints(self):
        atoms = set()
        for con in self.instance_constraints:
            atoms |= con.atoms(sm.Function)
        self.instance_constraint_function_atoms = atoms

    def _find_closest_free_index(self):
        N, n = self.num_collocation_nodes, self.num_states
        node_map = {}
        time_vector = None
        for func in self.instance_constraint_function_atoms:
            arg = func.args[0]
            if self._variable_duration:
                if arg == 0:
                    time_idx = 0
                else:
                    try:
                        time_idx = int(arg/self.time_interval_symbol)
                    except TypeError as err:
                        raise TypeError(
                            'Instance constraint {} is not a correct integer '
                            'multiple of the time interval.'.format(func)
                        ) from err
                if time_idx not in range(N):
                    raise ValueError(
                        'Instance constraint {} gives an index of {} which '
                        'is not between 0 and {}.'.format(func, time_idx,
                                                          N - 1))
            else:
                if time_vector is None:
                    time_vector = np.linspace(
                        0.0, self.node_time_interval*(N - 1), num=N)
                time_idx = int(np.argmin(np.abs(time_vector - float(arg))))
            base = func.__class__(self.time_symbol)
            if base in self.state_symbols:
                row = self.state_symbols.index(base)
            elif base in self.unknown_input_trajectories:
                row = n + self.unknown_input_trajectories.index(base)
            else:
                raise ValueError(f'{func} in an instance constraint is '
                                 'neither a state nor an unknown input '
                                 'trajectory.')
            node_map[func] = time_idx + row*N
        self.instance_constraints_free_index_map = node_map

    def _order_instance_atoms(self):
        """Fixes a deterministic atom order (by free index).  The reference
        iterates ``con.atoms(sm.Function)``, a set, so its order is only
        defined for single-atom constraints; those agree."""
        idx = self.instance_constraints_free_index_map
        self._inst_atoms = sorted(idx, key=lambda f: (idx[f], str(f)))
        per_con = []
        rows, cols = [], []
        base = self.num_eom*(self.num_collocation_nodes - 1)
        for i, con in enumerate(self.instance_constraints):
            atoms = sorted(con.atoms(sm.Function),
                           key=lambda f: (idx[f], str(f)))
            per_con.append(atoms)
            rows += [base + i]*len(atoms)
            cols += [idx[f] for f in atoms]
        self._inst_atoms_per_constraint = per_con
        self._inst_rows = np.array(rows, dtype=np.int64)
        self._inst_cols = np.array(cols, dtype=np.int64)

    def _instance_constraints_jacobian_indices(self):
        return self._inst_rows.copy(), self._inst_cols.copy()

    # ------------------------------------------------------------------
    # HIP program (replaces opty/direct_collocation.py:2304-2380, :2692-2814)
    # ------------------------------------------------------------------
    def _wrt(self):
        if self.integration_method == 'backward euler':
            wrt = (self.current_discrete_state_symbols +
                   self.previous_discrete_state_symbols +
                   self.current_unknown_discrete_specified_symbols +
                   self.unknown_parameters)
        else:
            wrt = (self.current_discrete_state_symbols +
                   self.next_discrete_state_symbols +
                   self.current_unknown_discrete_specified_symbols +
                   self.next_unknown_discrete_specified_symbols +
                   self.unknown_parameters)
        if self._variable_duration:
            wrt += (self.time_interval_symbol,)
        return wrt

    def _instance_placeholders(self, with_free_index=False):
        """The instance constraints written over one placeholder Symbol per
        function atom, as the program builders take them: ``(expressions,
        atom symbols, atoms per expression[, free index per atom])``; None
        without instance constraints."""
        if self.instance_constraints is None:
            return None
        place = {f: sm.Symbol('opty_atom_%d' % a, real=True)
                 for a, f in enumerate(self._inst_atoms)}
        exprs = [sm.sympify(c).xreplace(place)
                 for c in self.instance_constraints]
        grads = [[place[f] for f in atoms]
                 for atoms in self._inst_atoms_per_constraint]
        instance = (exprs, [place[f] for f in self._inst_atoms], grads)
        if with_free_index:
            instance += (self._atom_free_index(),)
        return instance

    def _builder_arguments(self):
        """The positional arguments the three program builders share (up to
        and including ``method``)."""
        be = self.integration_method == 'backward euler'
        return (list(self.discrete_eom),
                self.current_discrete_state_symbols,
                self.previous_discrete_state_symbols if be
                else self.next_discrete_state_symbols,
                self.current_discrete_specified_symbols,
                self.next_discrete_specified_symbols,
                self.num_known_input_trajectories,
                self.parameters, self.num_known_parameters,
                self.time_interval_symbol, self._variable_duration,
                self._wrt(), self.integration_method)

    def _build_program(self):
        if self._program is not None:
            return self._program
        logger.info('Lowering and differentiating the constraint function.')
        self._program = build_program(
            *self._builder_arguments(), self._instance_placeholders(),
            implicit=self._implicit_chain(), prune_zeros=self._prune_zeros,
            layout='csr' if self._jacobian_layout == 'csr' else 'coo')
        return self._program

    def _build_hessian_program(self):
        """The Hessian program of the constraint Lagrangian
        (:func:`opty_amd.codegen.program.build_hessian_program`), built on
        first use.  Problems whose second derivatives are not available are
        refused: implicit known trajectories (only ``dr/dx`` is given) and
        known trajectories given as functions of ``free``."""
        if getattr(self, '_hessian_program', None) is not None:
            return self._hessian_program
        if any(callable(v) for v in self.known_trajectory_map.values()):
            raise NotImplementedError(
                'the Hessian of a problem with known trajectories given as '
                'functions of the free vector is not available.')
        logger.info('Lowering and differentiating the constraint '
                    'Lagrangian twice.')
        self._hessian_program = build_hessian_program(
            *self._builder_arguments(),
            self._instance_placeholders(with_free_index=True),
            implicit=self._implicit_chain())
        return self._hessian_program

    #: operations per strip of ``opty_hess`` in the first build; halved (and
    #: chunks made to recompute what they share) while a build spills
    _HESS_STRIP_OPS = 1500

    def _build_hessian_code_object(self):
        """``(hsaco, strips, verdict)`` of the Hessian module: the first
        build whose kernels spill no vector register (smaller strips, then
        chunks that recompute what they share), through the static ISA check
        (a hit: the uniform-sincos sibling is built in its place when it is
        clean).  A module that spills whatever the cut is refused."""
        from .codegen.emit_hessian import emit_hessian_module
        hsaco, cut, meta = bl.spill_free_module(
            emit_hessian_module, self._build_hessian_program(), self._compile,
            ('opty_hess', 'opty_hess_inst'), self._HESS_STRIP_OPS)
        if hsaco is None:
            raise hb.HipBackendError(
                'every build of the Hessian kernels spills vector registers: '
                '%s' % meta['tried'])
        return hsaco, cut, dict(meta, strips=len(cut))

    #: constraint nodes the referee compares: the first wave and the last node
    _HESS_VERIFY_NODES = 64

    def _verify_hessian(self, handle):
        """Holds a Hessian build to its expression DAG before first use: the
        kernels, on random ``free`` and ``lagrange`` in device buffers that
        start as NaN, against the DAG as an instruction tape on the GPU
        (``opty_hip_tape_run``) on a node window, to 64 units of each entry's
        own rounding-error bound.  Raises :class:`hip_backend.BuildRejected`."""
        prog = self._build_hessian_program()
        N = self.num_collocation_nodes
        ncn = N - 1
        rng = np.random.default_rng(17)
        free = rng.uniform(-1.0, 1.0, self.num_free)
        if self._variable_duration:
            free[-1] = 0.01
        lam = rng.uniform(-1.0, 1.0, self.num_constraints)
        d_free, d_lam = hb.DeviceVector(free, self._device), \
            hb.DeviceVector(lam, self._device)
        d_out = hb.DeviceVector(np.full(handle.nnz, np.nan), self._device)
        try:
            handle.evaluate(d_free, d_lam, d_out, hb.DEVICE)
            self._hip.synchronize()
            got = d_out.numpy()
        finally:
            for v in (d_free, d_lam, d_out):
                v.close()
        nodes = np.unique(np.r_[np.arange(min(ncn, self._HESS_VERIFY_NODES)),
                                ncn - 1])
        inputs = self._hessian_inputs(free, lam, nodes)
        roots = list(prog.hess_out) + list(prog.inst_hess_out)
        val, bnd = self._tape_referee(prog, roots, inputs, len(nodes))
        PH = prog.PH
        worst = 0.0
        for e, (want, b) in enumerate(zip(val, bnd)):
            if e < PH:
                have = got[nodes*PH + e]
            else:
                t = e - PH
                scale = lam[prog.M*ncn + prog.inst_hess_con[t]]
                have = np.full(want.shape, got[ncn*PH + t])
                want, b = want*scale, b*abs(scale)
            worst = max(worst, self._tape_check(
                'Hessian entry %d' % e, have, want, b, np.abs(want),
                entry=e))
        return dict(ok=True, referee='tape', nodes=len(nodes),
                    worst_fraction_of_tolerance=worst)

    def _tape_referee(self, prog, roots, inputs, count):
        """Values of ``roots`` from the DAG of ``prog`` run as an instruction
        tape on the GPU (``opty_hip_tape_run``) at ``count`` nodes, and their
        rounding-error bounds: ``(len(roots), count)`` each."""
        from .codegen.tape import Tape
        from .codegen.errbound import evaluate_with_error_bound
        if not roots:
            return np.zeros((0, count)), np.zeros((0, count))
        tape = Tape(prog.dag, roots)
        vals = hb.tape_run(tape, tape.table(count, inputs), self._device)
        _, bound = evaluate_with_error_bound(prog.dag, roots, inputs)
        val = np.stack([vals[tape.slot[r]] for r in roots])
        bnd = np.stack([np.broadcast_to(np.abs(np.asarray(
            b, dtype=float)), (count,)) for b in bound])
        return val, bnd

    @staticmethod
    def _tape_check(subject, have, want, bnd, mag, **key):
        """Holds ``have`` to the referee's ``want``: 64 units of the entries'
        own rounding-error bounds ``bnd`` plus 4 units of ``mag``.  Returns
        the worst error as a fraction of the tolerance; raises
        :class:`hip_backend.BuildRejected` (its verdict: ``key`` and the
        error)."""
        u = 2.0**-53
        err = np.abs(have - want)
        tol = 64.0*u*bnd + 4.0*u*mag
        if not np.all(err <= tol):
            raise hb.BuildRejected(
                '%s disagrees with the instruction tape (max error %.3g)'
                % (subject, np.nanmax(err)),
                dict(key, err=float(np.nanmax(err))))
        return float(np.max(err/np.maximum(tol, 1e-300))) if err.size else 0.0

    def _hessian_inputs(self, free, lagrange, nodes):
        """``inputs(kind, index)`` of the Hessian DAG at the constraint nodes
        ``nodes`` (an index array) for ``free`` and ``lagrange``."""
        ncn = self.num_collocation_nodes - 1
        base = self._shared_inputs(self._build_hessian_program(), free, nodes)
        return lambda kind, k: lagrange[k*ncn + nodes] if kind == 'lam' \
            else base(kind, k)

    def _ensure_hessian(self):
        """The Hessian handle (built, checked and verified on first use; it
        borrows the problem handle's device data)."""
        def create(hip):
            prog = self._build_hessian_program()
            hsaco, cut, meta = self._build_hessian_code_object()
            rows, cols = self.hessian_indices_closed_form()
            PH, ncn = prog.PH, self.num_collocation_nodes - 1
            return hb.HipHessian(hip, dict(
                PH=PH, nnz_inst=len(prog.inst_hess_out),
                strips=max(1, len(cut)),
                pattern=np.array(prog.index_pattern(), dtype=np.int32),
                inst_rows=rows[ncn*PH:], inst_cols=cols[ncn*PH:]),
                hsaco), dict(meta, hsaco=hsaco)
        return self._ensure_derived('_hessian', create, self._verify_hessian)

    def _ensure_derived(self, attr, create, verify):
        """The handle ``self.<attr>`` of a derived program, made on first use:
        ``create(hip) -> (handle, meta)`` builds it on the problem handle,
        ``verify(handle)`` holds it to its DAG (a refused handle is
        released); ``self.<attr>_meta`` records ``meta`` and the verdict."""
        if getattr(self, attr, None) is not None:
            return getattr(self, attr)
        hip = self._ensure_hip()
        handle, meta = create(hip)
        self._sync_known(hip, None)
        try:
            verdict = verify(handle)
        except hb.BuildRejected:
            handle.release()
            raise
        setattr(self, attr + '_meta', dict(meta, verdict=verdict))
        setattr(self, attr, handle)
        return handle

    def generate_hessian_function(self):
        """Returns ``hessian(free, lagrange) -> ndarray``: the constraint part
        of the Hessian of the Lagrangian, ``sum_k lagrange_k d2 con_k /
        d free^2``, evaluated on the GPU, with ``lagrange`` ordered like
        ``constraints(free)`` (defects ``j*(N-1) + i``, then the instance
        constraints).  Values of the LOWER triangle as triplets, in the order
        of :meth:`hessian_indices`; a ``(row, col)`` pair may repeat and the
        matrix is the SUM of its triplets (IPOPT's convention and
        ``scipy.sparse.coo_matrix``'s; not the last-write-wins of the
        reference's Jacobian helper ``_coo_matrix``).  The result is a
        persistent page-locked buffer that the next call overwrites.

        ``free`` and ``lagrange`` may also be torch CUDA tensors; the result
        is then a new CUDA tensor (nothing crosses PCIe)."""
        handle = self._ensure_hessian()
        return self._derived_function(handle, handle.evaluate, 'lagrange',
                                      self.num_constraints, handle.nnz)

    def hessian_indices(self):
        """Row and column indices (int64, row >= col) of every value
        ``generate_hessian_function`` returns, in that order, from the
        device's closed form; pairs repeat (the matrix is the sum of its
        triplets)."""
        handle = self._ensure_hessian()
        rows = np.empty(handle.nnz, dtype=np.int64)
        cols = np.empty(handle.nnz, dtype=np.int64)
        handle.indices(rows, cols, hb.HOST)
        return rows, cols

    def hessian_indices_closed_form(self):
        """Row and column indices (int64) of the Hessian triplets from the
        closed form on the host (lower triangle; a pair may repeat and the
        matrix is the SUM of its triplets)."""
        from .codegen.program import hessian_indices
        idx = self.instance_constraints_free_index_map \
            if self.num_instance_constraints else {}
        return hessian_indices(self._build_hessian_program(),
                               self.num_collocation_nodes,
                               [idx[f] for f in self._inst_atoms])

    # ------------------------------------------------------------------
    # matrix-free Jacobian products
    # ------------------------------------------------------------------
    def _build_jacprod_program(self):
        """The Jacobian-product program
        (:func:`opty_amd.codegen.program.build_jacobian_product_program`),
        built on first use."""
        if getattr(self, '_jacprod_program', None) is not None:
            return self._jacprod_program
        logger.info('Lowering the tangent and the adjoint of the constraint '
                    'function.')
        self._jacprod_program = build_jacobian_product_program(
            *self._builder_arguments(), self._instance_placeholders(),
            implicit=self._implicit_chain())
        return self._jacprod_program

    def _atom_free_index(self):
        idx = self.instance_constraints_free_index_map \
            if self.num_instance_constraints else {}
        return [idx[f] for f in self._inst_atoms] if idx else []

    def _jacprod_inputs(self, free, vec, nodes, what):
        """``inputs(kind, index)`` of the product DAG at the constraint nodes
        ``nodes`` (an index array): ``what`` = ``'jvp'`` -- ``vec`` is the
        direction ``v`` -- or ``'vjp'`` -- ``vec`` is ``w``."""
        prog = self._build_jacprod_program()
        N = self.num_collocation_nodes
        ncn = N - 1
        base = self._shared_inputs(prog, free, nodes)
        vtail = vec[(prog.n + prog.q)*N:] if what == 'jvp' else None

        def inputs(kind, k):
            if kind in ('vcur', 'vadj'):
                src, r = prog.rows[k]
                assert src == 'free', (kind, k)
                off = prog.cur_offset if kind == 'vcur' else prog.adj_offset
                return vec[r*N:(r + 1)*N][nodes + off]
            if kind == 'vpar':
                return vtail[prog.pars[k][1]]
            if kind == 'vh':
                return vtail[prog.h[1]]
            if kind == 'lam':
                return vec[k*ncn + nodes]
            return base(kind, k)
        return inputs

    def _build_jacprod_block_program(self, columns=4):
        """The block product program of ``columns`` columns
        (:func:`opty_amd.codegen.program.build_jacobian_block_product_program`),
        built on first use, one per width."""
        from .codegen.program import build_jacobian_block_product_program
        cache = self.__dict__.setdefault('_jacprod_block_programs', {})
        if columns not in cache:
            logger.info('Lowering %d tangents and %d adjoints of the '
                        'constraint function on one DAG.', columns, columns)
            cache[columns] = build_jacobian_block_product_program(
                *self._builder_arguments(), self._instance_placeholders(),
                implicit=self._implicit_chain(), columns=columns)
        return cache[columns]

    def _jacprod_block_inputs(self, free, vecs, nodes, what):
        """``inputs(kind, index)`` of a block product DAG at the constraint
        nodes ``nodes``: :meth:`_jacprod_inputs` per column, ``vecs[:, c]``
        the vector of the column the index names
        (:func:`opty_amd.codegen.ir.split_column`)."""
        from .codegen.ir import split_column
        per_column = [self._jacprod_inputs(free, vecs[:, c], nodes, what)
                      for c in range(vecs.shape[1])]

        def inputs(kind, k):
            c, k = split_column(kind, k)
            return per_column[c](kind, k)
        return inputs

    def _shared_inputs(self, prog, free, nodes):
        """``inputs(kind, index)`` for the kinds every program shares
        (``cur``, ``adj``, ``par``, ``h``, ``free``) at the nodes ``nodes``."""
        N = self.num_collocation_nodes
        n, q = prog.n, prog.q
        tail = free[(n + q)*N:]
        known = self._known_trajectory_array(free) \
            if self.num_known_input_trajectories else None
        kpar = [float(self.known_parameter_map[p])
                for p in self.known_parameters]
        idx = self.instance_constraints_free_index_map \
            if self.num_instance_constraints else {}

        def inputs(kind, k):
            if kind in ('cur', 'adj'):
                src, r = prog.rows[k]
                row = free[r*N:(r + 1)*N] if src == 'free' else known[r]
                off = prog.cur_offset if kind == 'cur' else prog.adj_offset
                return row[nodes + off]
            if kind == 'par':
                src, r = prog.pars[k]
                return kpar[r] if src == 'known' else tail[r]
            if kind == 'h':
                return self.node_time_interval if prog.h[0] == 'fixed' \
                    else tail[prog.h[1]]
            assert kind == 'free', kind
            return free[idx[self._inst_atoms[k]]]
        return inputs

    #: operations per strip of ``opty_jvp`` / ``opty_vjp`` in the first
    #: build; halved (then units made to recompute what they share) while a
    #: build spills
    _JACPROD_STRIP_OPS = 1500
    _JACPROD_KERNELS = ('opty_jvp', 'opty_jvp_inst', 'opty_vjp',
                        'opty_vjp_fin')

    def _build_jacprod_code_object(self):
        """``(hsaco, meta)`` of the product module: the first build whose
        kernels spill no vector register (smaller strips, then units that
        recompute what they share), through the static ISA check (a hit: the
        uniform-sincos sibling is built in its place when it is clean).  A
        module that spills whatever the cut is refused."""
        from .codegen.emit_jacprod import emit_jacprod_module
        hsaco, cuts, meta = bl.spill_free_module(
            emit_jacprod_module, self._build_jacprod_program(), self._compile,
            self._JACPROD_KERNELS, self._JACPROD_STRIP_OPS)
        if hsaco is None:
            raise hb.BuildRejected(
                'every build of the Jacobian-product kernels spills vector '
                'registers: %s' % meta['tried'], meta)
        return hsaco, dict(meta, jvp_strips=max(1, len(cuts[0])),
                           vjp_strips=max(1, len(cuts[1])))

    #: constraint nodes the referee compares: the first two blocks of
    #: ``opty_vjp`` (both sides of a block edge), the last two nodes and the
    #: nodes of the instance atoms
    _JACPROD_VERIFY_NODES = 128
    #: nodes per tape run of the tail columns' sums (all nodes, in chunks)
    _JACPROD_TAIL_CHUNK = 8192

    def _verify_jacprod(self, handle):
        """Holds a product build to its expression DAG before first use: both
        products, on random ``free``, ``v`` and ``w`` in device buffers that
        start as NaN, against the DAG as an instruction tape on the GPU
        (``opty_hip_tape_run``) on a node window -- the tail columns of ``J^T
        w`` on all nodes -- to 64 units of each entry's own rounding-error
        bound.  Raises :class:`hip_backend.BuildRejected`."""
        prog = self._build_jacprod_program()
        N = self.num_collocation_nodes
        ncn, M = N - 1, prog.M
        rng = np.random.default_rng(19)
        free = rng.uniform(-1.0, 1.0, self.num_free)
        if self._variable_duration:
            free[-1] = 0.01
        v = rng.uniform(-1.0, 1.0, self.num_free)
        w = rng.uniform(-1.0, 1.0, self.num_constraints)
        # (known trajectories given as functions of ``free``: those of THIS
        # free vector; the next product installs its own again)
        self._sync_known(self._hip, free)
        vecs = [hb.DeviceVector(x, self._device) for x in (free, v, w)]
        outs = [hb.DeviceVector(np.full(max(1, k), np.nan), self._device)
                for k in (self.num_constraints, self.num_free)]
        try:
            handle.jvp(vecs[0], vecs[1], outs[0], hb.DEVICE)
            handle.vjp(vecs[0], vecs[2], outs[1], hb.DEVICE)
            self._hip.synchronize()
            jv = outs[0].numpy()[:self.num_constraints]
            jtw = outs[1].numpy()[:self.num_free]
        finally:
            for x in vecs + outs:
                x.close()
        return self._referee_products(
            prog, prog.tan_out, prog.adj_out,
            lambda nodes, what: self._jacprod_inputs(
                free, v if what == 'jvp' else w, nodes, what), v, w, jv, jtw)

    def _referee_products(self, prog, tan_out, adj_out, inputs, v, w, jv,
                          jtw, subject=''):
        """Holds ``jv = J v`` and ``jtw = J^T w`` to the roots ``tan_out`` /
        ``adj_out`` of ``prog`` run as an instruction tape
        (:meth:`_verify_jacprod`'s scheme); ``inputs(nodes, what)``: the
        DAG's inputs at the constraint nodes ``nodes`` for ``what`` = ``'jvp'``
        / ``'vjp'``."""
        N = self.num_collocation_nodes
        ncn, M = N - 1, prog.M
        atoms = self._atom_free_index()
        extra = [ncn - 2, ncn - 1]
        for f in atoms:
            extra += [f % N - 1, f % N]
        nodes = np.unique(np.clip(np.r_[
            np.arange(min(ncn, self._JACPROD_VERIFY_NODES)),
            np.array(extra, dtype=np.int64)], 0, ncn - 1))
        worst = [0.0]

        def check(what, have, want, bnd, mag):
            what = subject + what
            worst[0] = max(worst[0], self._tape_check(what, have, want, bnd,
                                                      mag, what=what))

        def referee(roots, inputs, count):
            return self._tape_referee(prog, roots, inputs, count)

        # J v: the defect rows, then the instance rows
        fin = inputs(nodes, 'jvp')
        val, bnd = referee(list(tan_out), fin, len(nodes))
        for j in range(M):
            check('jvp equation %d' % j, jv[j*ncn + nodes], val[j], bnd[j],
                  np.abs(val[j]))
        ival, ibnd = referee(list(prog.inst_jac_out), fin, 1)
        ival, ibnd = ival[:, 0], ibnd[:, 0]
        for k in range(prog.num_inst):
            ts = [t for t, (kk, _) in enumerate(prog.inst_pairs) if kk == k]
            vk = np.array([v[atoms[prog.inst_pairs[t][1]]] for t in ts])
            terms = ival[ts]*vk
            check('jvp instance row %d' % k, jv[M*ncn + k], terms.sum(),
                  float((ibnd[ts]*np.abs(vk)).sum()),
                  (len(ts) + 1)*float(np.abs(terms).sum()))

        # J^T w: the trajectory rows on the window
        rin = inputs(nodes, 'vjp')
        val, bnd = referee(list(adj_out), rin, len(nodes))
        want, wb, mag = (np.zeros(self.num_free) for _ in range(3))
        seen = np.zeros(N + 1, dtype=bool)
        seen[nodes] = True
        pos = np.zeros(N + 1, dtype=np.int64)
        pos[nodes] = np.arange(len(nodes))
        p = np.arange(N)
        checked = ((p == ncn) | seen[p]) & ((p == 0) | seen[p - 1])
        has_lo, has_hi = checked & (p < ncn), checked & (p >= 1)
        mask = np.zeros(self.num_free, dtype=bool)
        for R, lo, hi in prog.row_columns():
            row = slice(R*N, (R + 1)*N)
            mask[row] = checked
            for k, has, shift in ((lo, has_lo, 0), (hi, has_hi, 1)):
                if k is None:
                    continue
                at = pos[p[has] - shift]
                want[row][has] += val[k][at]
                wb[row][has] += bnd[k][at]
                mag[row][has] += np.abs(val[k][at])
        for t, (k, a) in enumerate(prog.inst_pairs):
            wk = w[M*ncn + k]
            want[atoms[a]] += wk*ival[t]
            wb[atoms[a]] += abs(wk)*ibnd[t]
            mag[atoms[a]] += 2.0*abs(wk*ival[t])
            assert mask[atoms[a]]
        check('vjp trajectory rows', jtw[mask], want[mask], wb[mask],
              mag[mask])

        # ... and the tail columns: sums over ALL constraint nodes
        tails = prog.tail_columns()
        if tails:
            roots = [adj_out[k] for _, k in tails]
            tot, tb, tm = (np.zeros(len(tails)) for _ in range(3))
            for a in range(0, ncn, self._JACPROD_TAIL_CHUNK):
                part = np.arange(a, min(ncn, a + self._JACPROD_TAIL_CHUNK))
                val, bnd = referee(roots, inputs(part, 'vjp'), len(part))
                tot += val.sum(axis=1)
                tb += bnd.sum(axis=1)
                tm += np.abs(val).sum(axis=1)
            tail0 = (prog.n + prog.q)*N
            at = tail0 + np.array([j for j, _ in tails])
            # a sum of ncn terms, whatever its order: ncn units of the sum
            # of the magnitudes at the very most
            check('vjp tail columns', jtw[at], tot, tb, 0.25*ncn*tm)
        return dict(ok=True, referee='tape', nodes=len(nodes),
                    tail_nodes=ncn if tails else 0,
                    worst_fraction_of_tolerance=worst[0])

    def _ensure_jacprod(self):
        """The product handle (built, checked and verified on first use; it
        borrows the problem handle's device data)."""
        def create(hip):
            prog = self._build_jacprod_program()
            hsaco, meta = self._build_jacprod_code_object()
            return hb.HipJacobianProduct(hip, dict(
                jvp_strips=meta['jvp_strips'], vjp_strips=meta['vjp_strips'],
                num_tail=prog.r + prog.s, nnz_inst=len(prog.inst_jac_out)),
                hsaco), dict(meta, hsaco=hsaco)
        return self._ensure_derived('_jacprod', create, self._verify_jacprod)

    _JACPROD_BLOCK_KERNELS = ('opty_jvp_block', 'opty_jvp_block_inst',
                              'opty_vjp_block', 'opty_vjp_block_fin')
    #: columns per pass of the block kernels, widest first
    _JACPROD_BLOCK_WIDTHS = (4, 2)

    def _build_jacprod_block_code_object(self):
        """``(hsaco, meta)`` of the block product module: the widest of
        ``_JACPROD_BLOCK_WIDTHS`` that has a build without vector spills --
        each width through the ladder of :meth:`_build_jacprod_code_object`.
        ``meta['width']`` is the module's width, ``meta['tried']`` the builds
        of every width met; when every one spills ``hsaco`` is None and the
        width 1: block calls then loop over the single kernels."""
        from .codegen.emit_jacprod import emit_jacprod_block_module
        tried = {}
        for width in self._JACPROD_BLOCK_WIDTHS:
            hsaco, cuts, meta = bl.spill_free_module(
                emit_jacprod_block_module,
                self._build_jacprod_block_program(width), self._compile,
                self._JACPROD_BLOCK_KERNELS, self._JACPROD_STRIP_OPS)
            if hsaco is None:
                tried[width] = meta['tried']
                continue
            return hsaco, dict(meta, width=width, tried=tried,
                               jvp_strips=max(1, len(cuts[0])),
                               vjp_strips=max(1, len(cuts[1])))
        logger.warning('every build of the block product kernels spills '
                       'vector registers (%s): block products go column by '
                       'column through the single kernels', tried)
        return None, dict(width=1, tried=tried)

    def _verify_jacprod_block(self, handle):
        """Holds a block build to its expression DAG before first use:
        :meth:`_verify_jacprod`'s scheme per column, on ``width`` distinct
        random columns of ``V`` and ``W`` -- one pass with all columns active
        and one with ``width - 1`` -- into device buffers that start as NaN
        and whose leading dimension is larger than the column: what lies
        between the columns, and the column past ``ncols``, must still be
        NaN.  Raises :class:`hip_backend.BuildRejected`."""
        K = handle.width
        prog = self._build_jacprod_block_program(K)
        nfree, ncon = self.num_free, self.num_constraints
        rng = np.random.default_rng(29)
        free = rng.uniform(-1.0, 1.0, nfree)
        if self._variable_duration:
            free[-1] = 0.01
        V = rng.uniform(-1.0, 1.0, (nfree, K))
        W = rng.uniform(-1.0, 1.0, (ncon, K))
        self._sync_known(self._hip, free)
        pad = 5
        ldy, ldg = ncon + pad, nfree + pad
        vecs = [hb.DeviceVector(x, self._device)
                for x in (free, V.T, W.T)]
        outs = [hb.DeviceVector(np.full(K*ld, np.nan), self._device)
                for ld in (ldy, ldg, ldy, ldg)]
        try:
            handle.jvp_block(vecs[0], vecs[1], nfree, outs[0], ldy, K,
                             hb.DEVICE)
            handle.vjp_block(vecs[0], vecs[2], ncon, outs[1], ldg, K,
                             hb.DEVICE)
            handle.jvp_block(vecs[0], vecs[1], nfree, outs[2], ldy, K - 1,
                             hb.DEVICE)
            handle.vjp_block(vecs[0], vecs[2], ncon, outs[3], ldg, K - 1,
                             hb.DEVICE)
            self._hip.synchronize()
            Y, G, Y1, G1 = (x.numpy().reshape(K, -1) for x in outs)
        finally:
            for x in vecs + outs:
                x.close()
        for name, full, part, n in (('jvp', Y, Y1, ncon), ('vjp', G, G1,
                                                           nfree)):
            if not (np.all(np.isnan(full[:, n:])) and
                    np.all(np.isnan(part[:, n:]))):
                raise hb.BuildRejected(
                    'block %s wrote between two result columns' % name,
                    dict(what=name))
            if not np.all(np.isnan(part[K - 1])):
                raise hb.BuildRejected(
                    'block %s stored a column past ncols' % name,
                    dict(what=name))
            if not np.array_equal(part[:K - 1, :n].view(np.int64),
                                  full[:K - 1, :n].view(np.int64)):
                raise hb.BuildRejected(
                    'block %s: a pass of %d columns and one of %d disagree'
                    % (name, K, K - 1), dict(what=name))
        worst, verdict = 0.0, {}
        for c in range(K):
            verdict = self._referee_products(
                prog, prog.tan_out[c], prog.adj_out[c],
                lambda nodes, what: self._jacprod_block_inputs(
                    free, V if what == 'jvp' else W, nodes, what),
                V[:, c], W[:, c], Y[c, :ncon], G[c, :nfree],
                subject='column %d: ' % c)
            worst = max(worst, verdict['worst_fraction_of_tolerance'])
        return dict(verdict, columns=K, worst_fraction_of_tolerance=worst)

    def _ensure_jacprod_block(self):
        """The block product handle (built, checked and verified on first
        use), or None when every block build spills: the block width is then
        1 and block calls loop over the single kernels."""
        if getattr(self, '_jacprod_block_width', None) == 1:
            return None

        class NoModule(Exception):
            pass

        def create(hip):
            hsaco, meta = self._build_jacprod_block_code_object()
            if hsaco is None:
                raise NoModule(meta)
            prog = self._build_jacprod_block_program(meta['width'])
            return hb.HipJacobianBlockProduct(hip, dict(
                width=meta['width'], jvp_strips=meta['jvp_strips'],
                vjp_strips=meta['vjp_strips'], num_tail=prog.r + prog.s,
                nnz_inst=len(prog.inst_jac_out)), hsaco), \
                dict(meta, hsaco=hsaco)
        try:
            handle = self._ensure_derived('_jacprod_block', create,
                                          self._verify_jacprod_block)
        except NoModule as none:
            self._ensure_jacprod()
            self._jacprod_block_meta = dict(
                none.args[0], hsaco=None,
                verdict=self._jacprod_meta['verdict'])
            self._jacprod_block_width = 1
            return None
        self._jacprod_block_width = handle.width
        return handle

    def _generate_block_product(self, which):
        handle = self._ensure_jacprod_block()
        single = self._generate_product(which)
        hip = self._hip
        nfree = self.num_free
        name, nin, nout = ('V', nfree, self.num_constraints) \
            if which == 'jvp' else ('W', self.num_constraints, nfree)
        launch = None if handle is None else \
            handle.jvp_block if which == 'jvp' else handle.vjp_block

        def evaluate(free, X):
            return call_block(launch, (free, 'free', nfree), (X, name, nin),
                              nout, hip.synchronize, self._sync_free, single)
        evaluate.handle = handle
        evaluate.width = 1 if handle is None else handle.width
        return evaluate

    def generate_jvp_block_function(self):
        """Returns ``jmm(free, V) -> ndarray (num_constraints, k)``: ``J(free)
        V`` for the ``k`` columns of ``V`` (shape ``(num_free, k)``) in one
        call.  The block kernels take ``jmm.width`` columns per pass and
        evaluate what does not depend on the column once per pass (DESIGN.md
        section 10.1); with width 1 -- every block build spills -- and for ``k
        == 1`` the columns go through :meth:`generate_jvp_function`, whose
        bits they then have.  A NumPy ``V`` in either memory order is
        converted once to column-major; the result is a new column-major
        float64 array, bit-identical from call to call.

        ``free`` and ``V`` may also be torch CUDA tensors; the result is then
        a new CUDA tensor (nothing crosses PCIe)."""
        return self._generate_block_product('jvp')

    def generate_vjp_block_function(self):
        """Returns ``jtmm(free, W) -> ndarray (num_free, k)``: ``J(free)^T W``
        for the ``k`` columns of ``W`` (shape ``(num_constraints, k)``);
        otherwise as :meth:`generate_jvp_block_function`."""
        return self._generate_block_product('vjp')

    def _generate_product(self, which):
        handle = self._ensure_jacprod()
        nfree, ncon = self.num_free, self.num_constraints
        if which == 'jvp':
            return self._derived_function(handle, handle.jvp, 'v', nfree,
                                          ncon)
        return self._derived_function(handle, handle.vjp, 'w', ncon, nfree)

    def _derived_function(self, handle, launch, name, nin, nout):
        """``f(free, vec) -> result`` over ``launch(free, vec, out, memory
        kind)`` of a derived handle: host arrays in, a persistent page-locked
        buffer of ``nout`` values out -- or torch CUDA tensors in, a new CUDA
        tensor out; ``vec`` is called ``name`` and has ``nin`` values."""
        hip = self._hip
        nfree = self.num_free
        result = hb.pinned_empty(nout)

        def evaluate(free, vec):
            return call_vectors(
                launch, ((free, 'free', nfree), (vec, name, nin)), result,
                hip.synchronize, before=self._sync_free)
        evaluate.handle = handle
        return evaluate

    def generate_jvp_function(self):
        """Returns ``jvp(free, v) -> ndarray (num_constraints,)``: the
        constraint Jacobian at ``free`` times ``v``, evaluated on the GPU
        without forming the matrix; ordered like ``constraints(free)``.  The
        matrix is the one of :meth:`jacobian_indices` and
        ``generate_jacobian_function`` (the SUM of its triplets), whatever
        ``prune_zeros`` and ``jacobian_layout`` are.  The result is a
        persistent page-locked buffer that the next call overwrites.

        ``free`` and ``v`` may also be torch CUDA tensors; the result is then
        a new CUDA tensor (nothing crosses PCIe)."""
        return self._generate_product('jvp')

    def generate_vjp_function(self):
        """Returns ``vjp(free, w) -> ndarray (num_free,)``: the transposed
        constraint Jacobian at ``free`` times ``w`` (``w`` ordered like
        ``constraints(free)``), ordered like ``free``; otherwise as
        :meth:`generate_jvp_function`.  Bit-identical from call to call."""
        return self._generate_product('vjp')

    def jacobian_operator(self, free):
        """The constraint Jacobian at ``free`` as a
        ``scipy.sparse.linalg.LinearOperator`` of shape ``(num_constraints,
        num_free)``: ``matvec`` / ``rmatvec`` are :meth:`generate_jvp_function`
        / :meth:`generate_vjp_function` at that ``free`` (a copy is kept; a
        torch CUDA tensor stays on the device), ``matmat`` / ``rmatmat`` one
        block product each (:meth:`generate_jvp_block_function` /
        :meth:`generate_vjp_block_function`).  Every product returns a new
        array."""
        from scipy.sparse.linalg import LinearOperator
        if getattr(self, '_jacprod_functions', None) is None:
            self._jacprod_functions = (self.generate_jvp_function(),
                                       self.generate_vjp_function())
        jvp, vjp = self._jacprod_functions
        if getattr(self, '_jacprod_block_functions', None) is None:
            self._jacprod_block_functions = (
                self.generate_jvp_block_function(),
                self.generate_vjp_block_function())
        jmm, jtmm = self._jacprod_block_functions
        if on_device(free):
            import torch
            free = free.detach().clone()

            def apply(f, x):
                # (the function takes a host vector to ``free``'s device)
                return f(free, np.reshape(x, -1)).cpu().numpy()

            def apply_block(f, X):
                if on_device(X):
                    return f(free, X)
                X = torch.from_numpy(column_major(X).T).to(free.device).t()
                return f(free, X).cpu().numpy()
        else:
            free = self._host_free(free).copy()

            def apply(f, x):
                return np.array(f(free, np.asarray(x).reshape(-1)))

            def apply_block(f, X):
                if on_device(X):
                    import torch
                    return torch.from_numpy(np.ascontiguousarray(
                        f(free, X.detach().cpu().numpy()))).to(X.device)
                return f(free, X)

        class JacobianOperator(tensor_operands('matmat', 'rmatmat'),
                               LinearOperator):
            """``matmat`` / ``rmatmat`` are one block product each
            (:meth:`generate_jvp_block_function`); a CUDA block of vectors is
            taken as it is (SciPy would convert it to an array) and answered
            with a CUDA tensor."""

            def __init__(op):
                super().__init__(np.dtype(np.float64),
                                 (self.num_constraints, self.num_free))

            def _matvec(op, x):
                return apply(jvp, x)

            def _rmatvec(op, x):
                return apply(vjp, x)

            def _matmat(op, X):
                return apply_block(jmm, X)

            def _rmatmat(op, X):
                return apply_block(jtmm, X)

        return JacobianOperator()

    # ------------------------------------------------------------------
    # Hessian operator: H v from the stored triplets
    # ------------------------------------------------------------------
    def _hessmv_descriptor(self, objective=None):
        """Descriptor of a :class:`hip_backend.HipHessianProduct` over the
        constraint triplets and, with ``objective`` (a
        :class:`hip_backend.HipObjectiveHessian`), the objective's behind
        them."""
        prog = self._build_hessian_program()
        rows, cols = self.hessian_indices_closed_form()
        N = self.num_collocation_nodes
        at = (N - 1)*prog.PH
        desc = dict(pattern=np.array(prog.index_pattern(), dtype=np.int32),
                    inst_rows=rows[at:], inst_cols=cols[at:])
        if objective is not None:
            tail = (prog.n + prog.q)*N
            desc.update(obj_pattern=objective.pattern,
                        obj_base=objective.desc['base'],
                        tail_rows=tail + objective.tail_pairs[:, 0],
                        tail_cols=tail + objective.tail_pairs[:, 1])
        return desc

    def _ensure_over_triplets(self, stem, cls, objective):
        """The handle of class ``cls`` over the Hessian's triplets (made on
        first use; ``self.<stem>`` for the constraint triplets alone,
        ``self.<stem>_objective`` with those of the objective Hessian handle
        ``self.<stem>_objective_of`` behind them: one per such handle)."""
        attr = stem if objective is None else stem + '_objective'
        if objective is not None and \
                getattr(self, attr + '_of', None) is not objective:
            old = getattr(self, attr, None)
            if old is not None:
                old.release()
            setattr(self, attr, None)
            setattr(self, attr + '_of', objective)

        def create(hip):
            return cls(hip, self._hessmv_descriptor(objective)), {}
        # (no program of its own to hold the kernels to: the handle is
        # checked against NumPy and scipy.sparse on the triplets by the test
        # suite)
        return self._ensure_derived(attr, create, lambda handle: None)

    def _ensure_hessmv(self, objective=None):
        """The Hessian-product handle."""
        return self._ensure_over_triplets('_hessmv', hb.HipHessianProduct,
                                          objective)

    def _hessmv_function(self, handle):
        """``hmv(values, v) -> y`` over ``handle``."""
        hip = self._hip
        nfree, nnz = self.num_free, handle.nnz
        result = hb.pinned_empty(nfree)

        def evaluate(values, v):
            return call_vectors(
                handle.apply, ((values, 'values', nnz), (v, 'v', nfree)),
                result, hip.synchronize)
        evaluate.handle = handle
        return evaluate

    def _hessmm_function(self, handle):
        """``hmm(values, V) -> Y`` over ``handle``, ``V`` of shape
        ``(num_free, k)``."""
        hip = self._hip
        nfree, nnz = self.num_free, handle.nnz

        def evaluate(values, V):
            return call_block(handle.apply_block, (values, 'values', nnz),
                              (V, 'V', nfree), nfree, hip.synchronize)
        evaluate.handle = handle
        return evaluate

    def generate_hessian_block_product_function(self):
        """Returns ``hmm(values, V) -> ndarray (num_free, k)``: ``H V`` on
        the GPU for the ``k`` columns of ``V`` in one call, ``H`` and
        ``values`` as for :meth:`generate_hessian_product_function`.  The
        handle takes ``handle.block_width`` columns per pass and reads every
        value once per pass; column ``c`` of the result has the bits of
        ``hmv(values, V[:, c])``.  A NumPy ``V`` in either memory order is
        converted once to column-major; the result is a new column-major
        float64 array.

        ``values`` and ``V`` may also be torch CUDA tensors; the result is
        then a new CUDA tensor of shape ``(num_free, k)`` (nothing crosses
        PCIe)."""
        return self._hessmm_function(self._ensure_hessmv())

    def generate_hessian_product_function(self):
        """Returns ``hmv(values, v) -> ndarray (num_free,)``: ``H v`` on the
        GPU, ``H`` the symmetric matrix whose lower triangle is the SUM of
        the triplets ``values`` that the callable of
        :meth:`generate_hessian_function` returned (order of
        :meth:`hessian_indices`).  Every element of the result is written
        exactly once in a fixed order of operations: the same inputs give the
        same bits.  The result is a persistent page-locked buffer that the
        next call overwrites.

        ``values`` and ``v`` may also be torch CUDA tensors; the result is
        then a new CUDA tensor (nothing crosses PCIe)."""
        return self._hessmv_function(self._ensure_hessmv())

    def _hessian_operator(self, handle, values):
        """``LinearOperator`` over ``handle`` and the triplets ``values`` (a
        CUDA tensor the operator keeps, or host values that go to a device
        buffer of the operator's own)."""
        from scipy.sparse.linalg import LinearOperator
        nfree = self.num_free
        hip = self._hip
        if on_device(values):
            import torch
            dev = values.device

            def apply(x):
                host = not on_device(x)
                if host:
                    x = torch.from_numpy(
                        host_vector(np.reshape(x, -1), 'v', nfree))
                x = device_vector(x.reshape(-1), 'v', nfree, dev)
                out = torch.empty(nfree, dtype=torch.float64, device=dev)
                wait_for_torch(dev)
                handle.apply(values, x, out, hb.DEVICE)
                hip.synchronize()
                return out.cpu().numpy() if host else out

            def apply_block(X):
                host = not on_device(X)
                if host:
                    X = torch.from_numpy(host_block(X, 'X', nfree))
                X = device_block(X, 'X', nfree, dev)
                k = X.shape[0]
                out = torch.empty((k, nfree), dtype=torch.float64, device=dev)
                if k:
                    wait_for_torch(dev)
                    handle.apply_block(values, X, nfree, out, nfree, k,
                                       hb.DEVICE)
                    hip.synchronize()
                return out.cpu().numpy().T if host else out.t()
        else:
            values = hb.DeviceVector(values, self._device)
            d_v = hb.DeviceVector(np.zeros(nfree), self._device)
            d_y = hb.DeviceVector(np.zeros(nfree), self._device)

            def apply(x):
                like = x if on_device(x) else None
                if like is not None:
                    x = x.detach().cpu().numpy()
                d_v.assign(host_vector(np.reshape(x, -1), 'v', nfree))
                handle.apply(values, d_v, d_y, hb.DEVICE)
                hip.synchronize()
                if like is not None:
                    import torch
                    return torch.from_numpy(d_y.numpy()).to(like.device)
                return d_y.numpy()

            def apply_block(X):
                like = X if on_device(X) else None
                if like is not None:
                    X = X.detach().cpu().numpy()
                X = host_block(X, 'X', nfree)
                k = X.shape[1]
                d_X = hb.DeviceVector(X.T, self._device)
                d_Y = hb.DeviceVector(np.zeros(k*nfree), self._device)
                handle.apply_block(values, d_X, nfree, d_Y, nfree, k,
                                   hb.DEVICE)
                hip.synchronize()
                Y = d_Y.numpy().reshape(k, nfree).T
                if like is not None:
                    import torch
                    return torch.from_numpy(Y).to(like.device)
                return Y

        class HessianOperator(
                tensor_operands('matvec', 'rmatvec', 'matmat'),
                LinearOperator):
            """Symmetric; a torch CUDA vector, or a CUDA block of vectors of
            shape ``(num_free, k)``, is taken as it is (SciPy would convert
            it to an array) and answered with a CUDA tensor.  ``matmat`` is
            one block product: bit for bit the column stack of ``matvec``."""

            def __init__(self):
                super().__init__(np.dtype(np.float64), (nfree, nfree))

            def _matvec(self, x):
                return apply(x)

            _rmatvec = _matvec

            def _matmat(self, X):
                return apply_block(X)

            _rmatmat = _matmat
        op = HessianOperator()
        op.values = values
        op.handle = handle
        return op

    def hessian_operator(self, free, lagrange):
        """The constraint part of the Hessian of the Lagrangian at ``(free,
        lagrange)`` as a ``scipy.sparse.linalg.LinearOperator`` of shape
        ``(num_free, num_free)``.  The triplets are evaluated ONCE
        (:meth:`generate_hessian_function`) into a device buffer that the
        operator owns -- ``.values``; a later Hessian evaluation does not
        change its products --, and every ``matvec`` / ``rmatvec`` (the matrix
        is symmetric) is one :meth:`generate_hessian_product_function` call on
        them and returns a new array.  A torch CUDA ``free`` stays on the
        device; a torch CUDA vector is answered with a CUDA tensor."""
        if getattr(self, '_hessian_function', None) is None:
            self._hessian_function = self.generate_hessian_function()
        values = self._hessian_function(free, lagrange)
        # (a CUDA result is a new tensor already; the host result is the
        # function's persistent buffer and is copied to the device)
        return self._hessian_operator(self._ensure_hessmv(), values)

    # ------------------------------------------------------------------
    # Hessian as CSR: unique lower triangle
    # ------------------------------------------------------------------
    def _ensure_hesscsr(self, objective=None):
        """The CSR-Hessian handle."""
        return self._ensure_over_triplets('_hesscsr', hb.HipHessianCsr,
                                          objective)

    @staticmethod
    def _csr_structure_of(handle, rows, count):
        """``(indptr, indices)`` (int64) of ``count`` entries in ``rows``
        rows from ``handle``'s closed form."""
        indptr = np.empty(rows + 1, dtype=np.int64)
        indices = np.empty(count, dtype=np.int64)
        handle.structure(indptr, indices, hb.HOST)
        return indptr, indices

    def hessian_csr_structure(self):
        """``(indptr, indices)`` (int64, as :meth:`jacobian_csr_structure`)
        of the constraint part of the Hessian of the Lagrangian in
        compressed-sparse-row form: the lower triangle over ``num_free``
        rows, exactly the distinct ``(row, col)`` pairs of
        :meth:`hessian_indices`, rows ascending, columns ascending within a
        row.  The values of :meth:`generate_hessian_csr_function` are ``data``
        of ``scipy.sparse.csr_matrix((data, indices, indptr), shape=(num_free,
        num_free))`` as they are (``has_canonical_format``)."""
        # (what has no Hessian is refused before a device is asked for)
        self._build_hessian_program()
        self._ensure_hessian()
        handle = self._ensure_hesscsr()
        return self._csr_structure_of(handle, self.num_free,
                                      handle.nnz_unique)

    def _hessian_csr_compress(self, handle):
        """``compress(values) -> data`` over ``handle``: host triplets in, a
        persistent page-locked array out; a torch CUDA tensor in, a new CUDA
        tensor out."""
        hip = self._hip
        nnz, nu = handle.nnz, handle.nnz_unique
        result = hb.pinned_empty(nu)

        def compress(values):
            return call_vectors(handle.compress, ((values, 'values', nnz),),
                                result, hip.synchronize)
        compress.result = result
        return compress

    def generate_hessian_csr_function(self):
        """Returns ``hcsr(free, lagrange) -> ndarray (nnz_unique,)``: the
        constraint part of the Hessian of the Lagrangian as ``data`` of the
        CSR lower triangle of :meth:`hessian_csr_structure`, every pair
        once.  The triplets of :meth:`generate_hessian_function` are
        evaluated into a device buffer that the function owns and compressed
        on the GPU; the triplets of a pair are added in a fixed order (a pair
        with up to a few triplets: ascending position, the bits of
        ``np.add.at``), every element is stored exactly once: the same inputs
        give the same bits.  The result is a persistent page-locked buffer
        that the next call overwrites.

        ``free`` and ``lagrange`` may also be torch CUDA tensors; the result
        is then a new CUDA tensor (nothing crosses PCIe).  ``hcsr.compress(
        values)`` does the same for triplets the caller already holds."""
        self._build_hessian_program()
        hess = self._ensure_hessian()
        handle = self._ensure_hesscsr()
        hip = self._hip
        nfree, ncon = self.num_free, self.num_constraints
        compress = self._hessian_csr_compress(handle)
        own = {}

        def evaluate(free, lagrange):
            point = ((free, 'free', nfree), (lagrange, 'lagrange', ncon))
            if on_device(free):
                import torch
                free, lagrange = device_vectors(point)
                self._sync_free(free)
                values = own.get('torch')
                if values is None or values.device != free.device:
                    values = own['torch'] = torch.empty(
                        hess.nnz, dtype=torch.float64, device=free.device)
                wait_for_torch(free.device)
                hess.evaluate(free, lagrange, values, hb.DEVICE)
                return compress(values)
            free, lagrange = host_vectors(point)
            self._sync_free(free)
            if 'host' not in own:
                own['host'] = tuple(
                    hb.DeviceVector(np.zeros(k), self._device)
                    for k in (nfree, ncon, hess.nnz, handle.nnz_unique))
            d_free, d_lam, d_values, d_data = own['host']
            d_free.assign(free)
            d_lam.assign(lagrange)
            hess.evaluate(d_free, d_lam, d_values, hb.DEVICE)
            handle.compress(d_values, d_data, hb.DEVICE)
            hip.synchronize()
            return d_data.read_into(compress.result)
        evaluate.handle = handle
        evaluate.compress = compress
        return evaluate

    # ------------------------------------------------------------------
    # Augmented system as CSR
    # ------------------------------------------------------------------
    def _require_csr_layout(self, what):
        if self._jacobian_layout != 'csr':
            raise ValueError("%s needs jacobian_layout='csr'." % what)

    def _ensure_kktcsr(self, objective=None):
        """The augmented-system handle."""
        return self._ensure_over_triplets('_kktcsr', hb.HipKktCsr, objective)

    def kkt_csr_structure(self):
        """``(indptr, indices)`` (int64) of the lower triangle of the
        augmented system ``K = [[W + diag(sigma) + delta_w I, J^T], [J,
        -delta_c I]]`` -- ``W`` the constraint part of the Hessian of the
        Lagrangian, ``J`` the constraint Jacobian -- in compressed-sparse-row
        form over ``num_free + num_constraints`` rows.  Row ``r < num_free``:
        the columns of row ``r`` of :meth:`hessian_csr_structure` and the
        diagonal, stored whether or not a triplet lands on it; row ``num_free
        + k``: the columns of row ``k`` of :meth:`jacobian_csr_structure`,
        then the diagonal.  Every diagonal is the last entry of its row; the
        values of :meth:`generate_kkt_csr_function` are ``data`` of
        ``scipy.sparse.csr_matrix((data, indices, indptr))`` as they are
        (``has_canonical_format``).  Needs ``jacobian_layout='csr'``."""
        # (refused before a device is asked for)
        self._require_csr_layout('kkt_csr_structure')
        self._build_hessian_program()
        self._ensure_hessian()
        handle = self._ensure_kktcsr()
        return self._csr_structure_of(
            handle, self.num_free + self.num_constraints, handle.nnz_kkt)

    def _kkt_csr_assemble(self, handle):
        """``assemble(hess_values, jac_values, sigma=None, delta_w=0.0,
        delta_c=0.0) -> data`` over ``handle``: host arrays in, a persistent
        page-locked array out; torch CUDA tensors in, a new CUDA tensor
        out."""
        hip = self._hip
        nfree, nh, nj, nk = (self.num_free, handle.nnz, hip.nnz,
                             handle.nnz_kkt)
        result = hb.pinned_empty(nk)

        def assemble(hess_values, jac_values, sigma=None, delta_w=0.0,
                     delta_c=0.0):
            return call_vectors(
                handle.assemble,
                ((hess_values, 'hess_values', nh),
                 (jac_values, 'jac_values', nj), (sigma, 'sigma', nfree)),
                result, hip.synchronize, scalars=(delta_w, delta_c))
        assemble.result = result
        return assemble

    def _kkt_csr_function(self, handle, hessian_into):
        """``kkt(free, lagrange, ..., sigma, delta_w, delta_c) -> data`` over
        ``handle``; ``hessian_into(free, lagrange, values, *extra)`` fills
        the device buffer ``values`` with the Hessian's triplets."""
        hip = self._hip
        nfree, ncon = self.num_free, self.num_constraints
        assemble = self._kkt_csr_assemble(handle)
        own = {}

        def evaluate(free, lagrange, *extra, sigma=None, delta_w=0.0,
                     delta_c=0.0):
            point = ((free, 'free', nfree), (lagrange, 'lagrange', ncon),
                     (sigma, 'sigma', nfree))
            if on_device(free):
                import torch
                if sigma is not None:       # (the assembly converts it)
                    check_vector(*point[2])
                free, lagrange = device_vectors(point[:2])
                self._sync_free(free)
                bufs = own.get('torch')
                if bufs is None or bufs[0].device != free.device:
                    bufs = own['torch'] = tuple(
                        torch.empty(k, dtype=torch.float64,
                                    device=free.device)
                        for k in (handle.nnz, hip.nnz))
                values, jac = bufs
                wait_for_torch(free.device)
                hessian_into(free, lagrange, values, *extra)
                hip.eval_jac(free, jac, hb.DEVICE)
                return assemble(values, jac, sigma, delta_w, delta_c)
            free, lagrange, sigma = host_vectors(point)
            self._sync_free(free)
            if 'host' not in own:
                own['host'] = tuple(
                    hb.DeviceVector(np.zeros(k), self._device)
                    for k in (nfree, ncon, handle.nnz, hip.nnz, nfree,
                              handle.nnz_kkt))
            d_free, d_lam, d_values, d_jac, d_sigma, d_data = own['host']
            d_free.assign(free)
            d_lam.assign(lagrange)
            if sigma is not None:
                d_sigma.assign(sigma)
            hessian_into(d_free, d_lam, d_values, *extra)
            hip.eval_jac(d_free, d_jac, hb.DEVICE)
            handle.assemble(d_values, d_jac,
                            None if sigma is None else d_sigma, delta_w,
                            delta_c, d_data, hb.DEVICE)
            hip.synchronize()
            return d_data.read_into(assemble.result)
        evaluate.handle = handle
        evaluate.assemble = assemble
        return evaluate

    def generate_kkt_csr_function(self):
        """Returns ``kkt(free, lagrange, sigma=None, delta_w=0.0,
        delta_c=0.0) -> ndarray``: ``data`` of :meth:`kkt_csr_structure`, the
        lower triangle of the augmented system assembled on the GPU.  The
        triplets of :meth:`generate_hessian_function` and the Jacobian's
        values are evaluated into device buffers that the function owns and
        never leave the device.  An off-diagonal entry of the ``W`` block has
        the bits of :meth:`generate_hessian_csr_function`'s element, a
        diagonal is ``(h + sigma_r) + delta_w`` (``h`` = ``+0.0`` where no
        triplet lands), a Jacobian entry has the bits of
        ``generate_jacobian_function()(free)``, a diagonal of the constraint
        block is ``0.0 - delta_c``; the same inputs give the same bits.  The
        result is a persistent page-locked buffer that the next call
        overwrites.

        ``free``, ``lagrange`` and ``sigma`` may also be torch CUDA tensors;
        the result is then a new CUDA tensor (nothing crosses PCIe).
        ``kkt.assemble(hess_values, jac_values, sigma=None, delta_w=0.0,
        delta_c=0.0)`` does the same for values the caller already holds.
        Needs ``jacobian_layout='csr'``."""
        self._require_csr_layout('generate_kkt_csr_function')
        self._build_hessian_program()
        hess = self._ensure_hessian()
        handle = self._ensure_kktcsr()
        kkt = self._kkt_csr_function(
            handle, lambda free, lagrange, values: hess.evaluate(
                free, lagrange, values, hb.DEVICE))

        def evaluate(free, lagrange, sigma=None, delta_w=0.0, delta_c=0.0):
            return kkt(free, lagrange, sigma=sigma, delta_w=delta_w,
                       delta_c=delta_c)
        evaluate.handle = handle
        evaluate.assemble = kkt.assemble
        evaluate.__doc__ = 'data of kkt_csr_structure() at (free, lagrange).'
        return evaluate

    # ------------------------------------------------------------------
    # Normal matrix: a direct solve with the block-tridiagonal J D^-1 J^T
    # 
    # ------------------------------------------------------------------
    def generate_normal_solver(self):
        """Returns ``ns``, a :class:`opty_amd.normal.NormalSolver`: the
        direct solver with the constraint normal matrix ``S = Jc[:, :T]
        diag(1/d[:T]) Jc[:, :T]^T + delta_c I`` -- ``Jc`` the ``M(N-1)``
        collocation rows of the Jacobian, ``T = (n+q)N`` the trajectory part
        of ``free`` --, which is symmetric block tridiagonal when ordered by
        constraint node.  ``ns.factor(free, d=None, delta_c=0.0)`` evaluates
        the Jacobian into a device buffer of its own, forms ``S`` and
        factorises it on the GPU (block cyclic reduction with Cholesky
        factors); ``ns.factor_values(jac_values, ...)`` does the same for
        values the caller holds; ``ns.solve(r)`` applies ``S^-1`` to ``r`` of
        shape ``(M(N-1),)`` or ``(M(N-1), k)``; ``ns.blocks(jac_values,
        d=None, delta_c=0.0)`` returns ``(A, B)``, the blocks themselves;
        ``ns.workspace_bytes`` is the device memory of the factors.  A pivot
        that is not positive and finite raises ``numpy.linalg.LinAlgError``.

        The tail columns (unknown parameters, a free interval) and the
        instance rows are not part of ``S``: it is all of ``J D^-1 J^T``
        only for a problem that has neither, otherwise a preconditioner.
        Takes ``jacobian_layout`` ``'coo'`` and ``'csr'``, pruned or not;
        one solver per collocator."""
        if self._jacobian_layout not in ('coo', 'csr'):
            # (refused before a device is asked for)
            raise ValueError(
                "generate_normal_solver needs jacobian_layout='coo' or "
                "'csr', not %r." % self._jacobian_layout)
        if getattr(self, '_normal_solver', None) is None:
            prog = self._build_program()

            def create(hip):
                return hb.HipNormalSolver(hip, dict(
                    M=prog.M, layout=self._jacobian_layout,
                    pattern=prog.pattern)), {}
            # (no program of its own: the handle is held to the host
            # statement and to scipy.sparse by the test suite)
            handle = self._ensure_derived('_normal', create,
                                          lambda handle: None)
            from .normal import NormalSolver
            self._normal_solver = NormalSolver(self, handle)
        return self._normal_solver

    def normal_operator(self, free, d=None, delta_c=0.0):
        """``S^-1`` of :meth:`generate_normal_solver` at ``free`` as a
        symmetric ``scipy.sparse.linalg.LinearOperator`` of shape ``(M(N-1),
        M(N-1))``: ``S`` is factorised once, here, and every ``matvec`` /
        ``matmat`` is one ``ns.solve``.  The factors live in the collocator's
        solver: a product after a later factorisation raises
        ``RuntimeError``.  A torch CUDA vector is answered with a CUDA
        tensor."""
        solver = self.generate_normal_solver()
        solver.factor(free, d, delta_c)
        return solver.operator()

    def generate_source(self):
        """HIP source of this problem's kernels and its launch metadata."""
        return self._emit(self._printer_options())

    def _launch_blocks(self):
        nodes = self._launch_nodes or self.num_collocation_nodes - 1
        return (int(nodes) + 63)//64

    def _printer_options(self):
        opts = self._emit_options
        if opts is None:
            from . import launch_plan
            opts = launch_plan.lookup(self._build_program(),
                                      self._launch_blocks()) or EmitOptions()
        if self._deterministic and not opts.deterministic:
            import copy
            opts = copy.copy(opts)
            opts.deterministic = 1
        return opts

    def _compile(self, source, opt_level=None, extra_flags=()):
        """``hipcc --genco`` of one of this problem's modules (a
        ``deterministic`` collocator's without FMA contraction)."""
        if self._deterministic:
            extra_flags = tuple(extra_flags) + hb.DETERMINISTIC_FLAGS
        if 'opty_opaque(' in source:
            # modules with persistent kernels (dispatch order 'list')
            extra_flags = tuple(extra_flags) + hb.LOOP_FLAGS
        return hb.compile_module(source, self.tmp_dir,
                                 self.show_compile_output,
                                 opt_level=opt_level,
                                 extra_flags=tuple(extra_flags))

    def _emit(self, opts):
        return emit_module(self._build_program(), opts,
                           node_blocks=self._launch_blocks(),
                           literals=self._literals())

    def _known_scalars(self):
        """``(known parameter values, fixed interval or None)`` as the
        kernels get them."""
        par = tuple(float(self.known_parameter_map[p])
                    for p in self.known_parameters)
        h = None if self._variable_duration else \
            float(self.node_time_interval)
        return par, h

    def _literals(self):
        """``{node: value}`` of the node-invariant nodes of the program
        that do not depend on ``free``, for the CURRENT known parameter
        values (``specialize_parameters=True``), or None."""
        if not self._specialize:
            return None
        from .codegen.evaluate import evaluate_uniform
        from .codegen import ir
        prog = self._build_program()
        par, h = self._known_scalars()
        if self._specialized_for == (par, h) and \
                self._literal_values is not None:
            return self._literal_values
        d = prog.dag

        def scalar(kind, idx):
            if kind == 'par':
                src, k = prog.pars[idx]
                return par[k] if src == 'known' else None
            if kind == 'h':
                return h if prog.h[0] == 'fixed' else None
            return None

        roots = [i for i in d.reachable(
            set(prog.con_out) | set(prog.jac_out) |
            set(prog.inst_con_out or ()) | set(prog.inst_jac_out or ()))
            if d.uni[i] and d.op[i] != ir.CONST]
        vals = evaluate_uniform(d, roots, scalar)
        self._literal_values = {i: vals[i] for i in roots if i in vals}
        self._specialized_for = (par, h)
        return self._literal_values

    #: kernels of the restricted flavour (``emit_hip.emit_module``)
    _RESTRICTED_KERNELS = ('opty_jac_var', 'opty_conjac_var')

    def _build_code_object(self, opt_level=None):
        """:meth:`_build_checked`'s code object, with the verdict on its
        restricted kernels (``opty_jac_var`` / ``opty_conjac_var``: what
        evaluations into a registered output launch) in
        ``meta['restricted_ok']``.  They are an extra: a build in which one
        of them spills vector registers, carries the EXEC-copy pattern of
        the static ISA check, or sits next to a banned full kernel is used
        WITHOUT them (the descriptor says the module has none, registered
        outputs are written whole) -- never rebuilt for their sake."""
        hsaco, meta = self._build_checked(opt_level)
        if 'jac_var' not in meta['kernels']:
            return hsaco, meta
        if meta.get('banned_kernels'):
            why = 'full kernels banned: %s' % (meta['banned_kernels'],)
        else:
            why = bl.static_gate(hsaco, self._RESTRICTED_KERNELS).refusal()
        run_hsaco = None
        if why is None and meta.get('run'):
            # the run form of the two kernels: a code object of its own
            # (the module above is what it is without the form), held to
            # the same static gate; one that fails it is left out and the
            # dispatch form above serves
            run_hsaco = self._compile(meta['run']['source'],
                                      opt_level=opt_level)
            refused = bl.static_gate(
                run_hsaco, self._RESTRICTED_KERNELS).refusal()
            self._run_form_refused = refused
            if refused:
                logger.info('the run form of the restricted kernels of %s '
                            'is not used (%s)', os.path.basename(hsaco),
                            refused)
                run_hsaco = None
        meta = dict(meta, run_hsaco=run_hsaco)
        if why:
            logger.info('the restricted kernels of %s are not used (%s)',
                        os.path.basename(hsaco), why)
        return hsaco, dict(meta, restricted_ok=why is None,
                           restricted_refused=why)

    _FULL_KERNELS = ('opty_con', 'opty_jac', 'opty_conjac')

    def _build_checked(self, opt_level=None):
        """The code object this collocator uses, ``(hsaco, meta)``:
        :meth:`_build_spill_free`'s, unless the static ISA check
        (``opty_amd.isa_check``: a vector register copied into an
        accumulation register under a narrowed EXEC and read back under a
        wider one -- the hipcc 7.2 fault of DESIGN.md 4.1 that is understood
        at the instruction) finds such a copy in one of its kernels.  Then
        the same geometry printed with ``fast_trig=2`` (sincos behind a
        wave-uniform test: no EXEC-narrowing if / else on the hot path, which
        is where the copies sit) is built, and used when it is clean -- no
        such copy, no vector spills --, BEFORE any GPU time is spent on
        either.  ``meta['isa_exec_copies']`` carries
        the count of the build in use (None: the LLVM tools failed); the
        referee judges it like any other build.

        Before that: automatic parameter specialisation
        (``specialize_parameters=None``) -- when the generic module's fused
        kernel spills ``_AUTO_SPECIALIZE_SGPR_SPILLS`` scalar registers or
        more, the module with the known parameters printed as literals is
        built in its place (:meth:`_wants_auto_specialization`)."""
        build = self._build_spill_free(opt_level)
        if self._wants_auto_specialization(build.hsaco, opt_level):
            # the generic module of this problem is of the class that gains
            # from literals: build (and from here on use) the specialised one
            logger.info('the generic kernels spill %d scalar registers: '
                        'using parameter-specialised kernels '
                        '(specialize_parameters=None: automatic)',
                        hb.cached_kernel_resources(build.hsaco)[
                            'opty_conjac']['.sgpr_spill_count'])
            self._specialize = self._auto_specialized = True
            self._specialized_for = self._literal_values = None
            build = self._build_spill_free(opt_level)
        if self._auto_specialized:
            build = build._replace(
                meta=dict(build.meta, auto_specialized=True))
        build = self._uniform_sibling_if_better(build, opt_level)
        self._built_source, self._built_options = build.source, build.options
        return build.hsaco, build.meta

    def _uniform_sibling_if_better(self, build, opt_level):
        """``build`` through the static ISA check of its full kernels, or
        its clean ``fast_trig=2`` sibling (:meth:`_build_checked`)."""
        hsaco, meta = build.hsaco, build.meta
        banned = set(meta.get('banned_kernels', ()))
        gate = bl.static_gate(hsaco, self._FULL_KERNELS, ignore=banned,
                              spills=build.spills)
        if gate.error is not None:
            logger.warning('static ISA check of %s failed: %s', hsaco,
                           gate.error)
            return build._replace(meta=dict(meta, isa_exec_copies=None))
        hits = gate.copies
        build = build._replace(meta=dict(meta, isa_exec_copies=dict(hits)))
        if not hits or self._emit_options is not None or \
                self._pinned_build() is not None or \
                build.options.fast_trig == 2 or opt_level is not None:
            return build
        if isa_check.noted(hsaco, 'sibling_no_better'):
            # (found out by an earlier build of the same module)
            return build
        twin = self._trials().build(build.options, dict(fast_trig=2))
        spills = {k: v for k, v in twin.spills.items() if k not in banned}
        gate = bl.static_gate(twin.hsaco, self._FULL_KERNELS, ignore=banned,
                              spills=spills)
        if gate.error is not None:
            # (no note: a later build tries again)
            logger.info('static ISA check: %s in %s; its uniform-sincos '
                        'sibling could not be checked (%s): kept', hits,
                        os.path.basename(hsaco), gate.error)
            return build
        if not gate.clean:
            logger.info('static ISA check: %s in %s; the uniform-sincos '
                        'sibling is no better (copies %s, spills %s): kept',
                        hits, os.path.basename(hsaco), gate.copies, spills)
            isa_check.note(hsaco, 'sibling_no_better',
                           dict(copies=gate.copies, spills=spills))
            return build
        logger.info('static ISA check: %s in %s: replaced by the uniform-'
                    'sincos sibling %s (clean)', hits,
                    os.path.basename(hsaco), os.path.basename(twin.hsaco))
        keep = {k: meta[k] for k in ('banned_kernels', 'vector_spills',
                                     'auto_specialized') if k in meta}
        return twin._replace(meta=dict(
            twin.meta, isa_exec_copies={}, isa_replaced=dict(hits), **keep))

    #: spilled scalar registers of the generic fused kernel from which the
    #: parameter-specialised module is used automatically
    _AUTO_SPECIALIZE_SGPR_SPILLS = 200
    #: ... for blocks of at most this many entries per node
    _AUTO_SPECIALIZE_MAX_BLOCK = 1024

    def _wants_auto_specialization(self, hsaco, opt_level):
        if self._specialize_mode is not None or self._specialize or \
                self._auto_specialized is None or opt_level is not None or \
                self._emit_options is not None or self._deterministic or \
                not (self.num_known_parameters or
                     not self._variable_duration):
            return False
        if self._pinned_build() is not None:
            return False
        if self._build_program().P > self._AUTO_SPECIALIZE_MAX_BLOCK:
            # blocks this large are bound by their store stream, not by
            # their instructions (the 24-link stand-ins: -3 % for a second
            # compile of minutes)
            return False
        try:
            res = hb.cached_kernel_resources(hsaco)
            spilled = res['opty_conjac']['.sgpr_spill_count']
        except (KeyError, hb.HipBackendError):
            return False
        return spilled >= self._AUTO_SPECIALIZE_SGPR_SPILLS

    def _trials(self):
        return bl.TrialBuilder(self._emit, self._compile)

    def _build_spill_free(self, opt_level=None):
        """Emits and compiles this problem's module; returns the
        ``build_ladder.Build``.  Unless the caller fixed the printer options,
        a build whose kernels spill VECTOR registers to scratch memory is not
        used (see ``hip_backend.vgpr_spills``): the constraint rows are
        re-cut by count, then the strips of the spilling kernels are made
        narrower, until a build is spill-free
        (``build_ladder.spill_free``)."""
        trials = self._trials()
        pinned = self._pinned_build()
        if pinned is not None and opt_level is None:
            # a build that replaced one the verification refused
            # (_verified_alternative): reproduced exactly as recorded
            return trials.build(pinned[0], how=pinned[1])
        best = trials.build(self._printer_options(),
                            how=dict(opt_level=opt_level))
        if self._emit_options is not None:
            # the caller fixed the geometry: it is built as asked, but never
            # silently -- this is the build class that returned wrong values
            if best.spills:
                logger.warning(
                    'emit_options give kernels that spill vector registers '
                    'to scratch memory (%s); such builds have returned wrong '
                    'values (DESIGN.md 4.1): drop emit_options, or verify '
                    'with ConstraintCollocator.cross_check()', best.spills)
            return best
        best = bl.spill_free(trials, best, self._jacobian_layout)
        if best.spills and \
                set(best.spills) in ({'opty_jac'}, {'opty_conjac'}) and \
                self._jacobian_layout in ('coo', 'csr'):
            # ONE of the two Jacobian kernels spills whatever the cut, the
            # other is clean (the biped's 6 250-node shard: opty_jac, 2
            # registers): the spilling kernel is never launched -- the
            # handle routes its entry point through the clean one
            # (opty_hip_desc.routing: OPTY_HIP_ROUTE_NO_*), every wrong
            # build of r03 was of this class.
            banned = sorted(best.spills)
            logger.info('kernel %s spills vector registers whatever the cut '
                        '(%s): it will not be launched, %s serves its entry '
                        'point', banned[0], best.spills,
                        'opty_conjac' if banned == ['opty_jac']
                        else 'opty_con + opty_jac')
            return best._replace(meta=dict(
                best.meta, banned_kernels=banned,
                vector_spills=dict(best.spills)))
        if best.spills:
            # No cut is spill-free (a system larger than anything in the
            # zoo).  The wrong values of round 3 followed one stage of the
            # pre-RA scheduler, which only runs for such kernels; every build
            # of the repro without it was correct, 131 spilled registers or
            # not (profiles/r03_spill_incident.txt).  So the last resort is
            # the least-spilling cut built WITHOUT that stage -- and a loud
            # warning: run ``cross_check()`` on such a problem.
            hsaco = self._compile(
                best.source, extra_flags=hb.SAFE_SCHEDULER_FLAGS,
                opt_level=opt_level)
            logger.warning('kernels %s spill vector registers to scratch '
                           'memory whatever the cut (%d states, %d entries '
                           'per block, launches of %d blocks): built with %s; '
                           'verify with ConstraintCollocator.cross_check()',
                           best.spills, self.num_states, self._program.P,
                           self._launch_blocks(),
                           ' '.join(hb.SAFE_SCHEDULER_FLAGS))
            return best._replace(hsaco=hsaco)
        return best

    def _pinned_build(self):
        """``(EmitOptions, {'opt_level': .., 'extra_flags': ..})`` of the
        build that replaced one the verification refused -- found by this
        collocator (:meth:`_verified_alternative`) or recorded in the plan
        file (``"pinned"`` entries of ``launch_plans.json``) -- or None."""
        if self._emit_options is not None:
            return None
        if self._pinned is not None:
            return self._pinned
        from . import launch_plan
        entry = launch_plan.lookup_entry(self._build_program(),
                                         self._launch_blocks())
        if entry and entry.get('pinned') is not None:
            try:
                return EmitOptions(**entry['options']), dict(entry['pinned'])
            except (TypeError, AssertionError, KeyError):
                return None             # written by another printer version
        return None

    def _verified_alternative(self, refused, meta, err):
        """Another build of this problem's kernels that the verification
        accepts, after it refused ``refused`` (:meth:`_verify_build`).

        hipcc's faults at the register limit are erratic in the cut -- the
        biped's default 20 strips are wrong in strip 17, identically in both
        Jacobian kernels, while 12, 24 and 32 strips, 16-entry chunks and the
        other ``sincos`` are right -- so the neighbouring geometries
        (``build_ladder.neighbours``) are tried in the order of their
        expected cost (r05: first the same
        geometry with ``fast_trig=2``; strips +2, +4, +1, +6 ..., then
        ``fast_trig=1``, 16-entry chunks, then the same source through
        ``-O1`` and without the pre-RA stage of round 3), several compiled at
        a time, each held to the instruction tape; the first accepted one is
        used, remembered by this collocator and recorded in the plan file as
        a ``"pinned"`` entry (``__graft_entry__.build`` prebuilds those).
        Raises ``err`` when nothing passes."""
        from . import launch_plan
        base = self._built_options or self._printer_options()
        trials = self._trials()
        tried = [(os.path.basename(refused), err.verdict['errors'])]
        for batch in bl.batches(bl.neighbours(base, meta['geometry'],
                                              self._jacobian_layout)):
            for (label, _, _), build in zip(
                    batch, trials.build_all(base, batch)):
                hsaco = build.hsaco
                if hsaco == refused:
                    continue
                # (the referee reads the candidate's own source and options)
                self._built_source = build.source
                self._built_options = opts = build.options
                try:
                    verdict = self._verify_build(hsaco, build.meta,
                                                 force=True)
                except hb.BuildRejected as again:
                    tried.append((label, again.verdict['errors']))
                    continue
                logger.warning(
                    'the default build of this problem\'s kernels (%s) was '
                    'refused by the verification (%s); using %s (%s) instead',
                    os.path.basename(refused), err.verdict['errors'], label,
                    os.path.basename(hsaco))
                verdict = dict(verdict, replaces=os.path.basename(refused),
                               replacement=label, refused=tried)
                self._pinned = (opts, build.how)
                try:
                    launch_plan.record(
                        launch_plan.key_of(self._build_program(),
                                           self._launch_blocks()),
                        dict(options=launch_plan.options_kwargs(opts),
                             pinned=dict(build.how, label=label,
                                         replaces=os.path.basename(refused)),
                             refused=tried,
                             nodes=self._launch_nodes or
                             self.num_collocation_nodes - 1,
                             problem='%d states, %d entries per block'
                             % (self.num_states, self._program.P)))
                except OSError:
                    pass
                return hsaco, build.meta, verdict
        raise hb.BuildRejected(
            '%s  No neighbouring build passes either: %s' % (err, tried),
            err.verdict)

    def prebuild(self):
        """Builds what :meth:`_ensure_hip` will load, without a device: the
        code object of the printer's choice -- or, when the plan file holds a
        ``"pinned"`` entry for this problem (a build that replaced one the
        verification refused), exactly that one.  Returns ``(hsaco,
        meta)``."""
        return self._build_code_object()

    #: nodes the automatic check below evaluates (``verify_builds='off'``
    #: disables it; ``OPTY_CROSS_CHECK=hot`` -- or ``=off`` -- in the
    #: environment restricts it to builds at the register limit)
    _VERIFY_NODES = 199
    _VERIFY_RTOL = 1e-9
    #: disagreements up to this are re-examined on a second set of inputs
    #: (an ill-conditioned row), larger ones refuse the build at once
    _VERIFY_CONFIRM = 1e-6
    #: version of the referee a cached verdict must come from: 1 = host
    #: arrays (r04), 2 = register poison + device vectors of its own (r05),
    #: 3 = marginal disagreements settled by the entries' own rounding-error
    #: bounds on two seeds, not by the better of two seeds (r06)
    _REFEREE_VERSION = 3

    def _verify_build(self, hsaco, meta, force=False):
        """Holds a build to the expression DAG itself before the handle is
        handed out; raises :class:`hip_backend.BuildRejected` when a kernel
        disagrees.  Every build goes through it once (a fraction of a second
        next to the seconds of its compilation; the verdict is cached next to
        the code object); ``OPTY_CROSS_CHECK=hot`` restricts it to the builds
        that have actually failed -- kernels at the edge of the register file
        (``hip_backend.high_pressure_kernels``: >= 480 VGPRs or spilled
        SGPRs); ``=off`` in the environment means the same (those builds
        cannot be exempted from outside), only ``verify_builds='off'`` given
        to the constructor disables the check.

        Why: hipcc 7.2 has produced code objects of exactly such kernels
        whose values are wrong, deterministically and in whole strips:
        ``-O2`` schedules with vector spills in round 3, an
        ``-O1`` build WITHOUT vector spills in round 4 (504 VGPRs, 373
        spilled SGPRs: 2.7 % off in one strip), and then a spill-free ``-O2``
        build of the seven-segment biped whose separate AND fused kernels
        returned the same wrong strip, confirmed by a twin from another
        pipeline -- builds cannot vouch for each other.  The referee is
        ``opty_hip_tape_run``: the DAG as an instruction tape
        (``codegen/tape.py``) executed on the GPU by one small hand-written
        kernel of the runtime library, one lane per node, every value in
        HBM, the same device math library -- nothing for a register
        allocator to get wrong.  ``opty_con``, ``opty_jac`` and both outputs
        of ``opty_conjac`` must agree with it on the first ``_VERIFY_NODES``
        nodes (the first wave, two interior ones and a ragged last one; the
        kernels do not depend on N and every wrong build was wrong at every
        node) to ``_VERIFY_RTOL``
        of the largest value of the equation's row.  The verdict is
        remembered next to the code object (``<hsaco>.crosscheck.json``)."""
        import json
        import os
        mode = self._verify_mode
        if mode is None:
            # the environment may restrict the check to the class that has
            # failed (kernels at the register limit), it cannot switch it
            # off for that class: ``off`` there reads as ``hot``.  Opting
            # out altogether is an API decision (``verify_builds='off'``),
            # made where the collocator is made
            mode = os.environ.get('OPTY_CROSS_CHECK', '').lower()
            if mode == 'off':
                mode = 'hot'
        if mode == 'off':
            return None
        if hb.load_library().opty_hip_device_count() <= 0:
            return None         # creating the handle says what is missing
        hot = hb.high_pressure_kernels(hsaco)
        if not hot and mode == 'hot' and not force:
            return None
        side = hsaco + '.crosscheck.json'
        if meta.get('run_hsaco'):
            # (the verdict on a build that carries the run form of the
            # restricted kernels is a verdict on that code object as well)
            side = '%s.%s.crosscheck.json' % (hsaco, os.path.basename(
                meta['run_hsaco']).replace('.hsaco', ''))
        try:
            with open(side) as f:
                verdict = json.load(f)
            # (verdicts of an older referee are not trusted: the one without
            # register poison and device vectors of its own ACCEPTED two
            # faulty builds in r05)
            if verdict.get('ok') is True and verdict.get('referee') == 'tape' \
                    and verdict.get('referee_version') == \
                    self._REFEREE_VERSION:
                return verdict
        except (OSError, ValueError):
            pass
        logger.info('checking the build against the instruction tape%s',
                    ' (kernels at the register limit: %s)' % hot if hot
                    else '')
        # seeded inputs from (-1, 1); equations that are not finite there
        # (square roots, logarithms of states) are tried on narrower positive
        # ranges -- what stays non-finite must be non-finite in the build too
        for span in self._VERIFY_SPANS:
            rcon, rjac, con_row, jac_row = self._reference_values(span=span)
            if np.isfinite(rcon).all() and np.isfinite(rjac).all():
                break
        def compare(seed, floors=(None, None)):
            rcon, rjac, con_row, jac_row = self._reference_values(
                seed=seed, span=span)
            fcon, fjac = floors
            worst = {}
            # once per register poison (see _evaluate_build): a kernel that
            # reads a register it never wrote may come out right with ONE
            # pattern (the wrong-value counts of the frozen builds follow
            # the pattern: profiles/r05_poison_probe.txt)
            restricted = bool(self._restricted_geometry(meta)[
                'var_jac_wgs_per_block'])
            for pattern in hb.POISONS:
                con, jac, con2, jac2, *var = self._evaluate_build(
                    meta, hsaco, seed=seed, span=span, pattern=pattern,
                    restricted=restricted)
                got = {
                    'opty_con': self._row_error(con, rcon, con_row, fcon),
                    'opty_jac': self._row_error(jac, rjac, jac_row, fjac),
                    'opty_conjac': max(
                        self._row_error(con2, rcon, con_row, fcon),
                        self._row_error(jac2, rjac, jac_row, fjac))}
                if restricted:
                    # the restricted kernels, each into a registered buffer
                    # that the full kernel filled for ANOTHER free vector:
                    # compared whole, so a line they must write and do not
                    # shows as the other vector's value
                    jac3, con4, jac4 = var
                    got['opty_jac_var'] = self._row_error(jac3, rjac,
                                                          jac_row, fjac)
                    got['opty_conjac_var'] = max(
                        self._row_error(con4, rcon, con_row, fcon),
                        self._row_error(jac4, rjac, jac_row, fjac))
                worst = {k: max(v, worst.get(k, 0.0))
                         for k, v in got.items()}
            return worst

        errors = compare(7)
        worst = max(errors.values())
        marginal = None
        if self._VERIFY_RTOL < worst <= self._VERIFY_CONFIRM:
            # A small disagreement may be an ill-conditioned entry (a
            # cancellation, 1/x next to a pole) that the kernel's FMA
            # contraction and operation order round differently from the
            # one-operation-per-instruction tape -- or a small compiler
            # fault.  The two are told apart by the entry's OWN rounding-
            # error bound (codegen/errbound.py: a running error analysis of
            # the DAG at the verification inputs), not by looking for a
            # seed on which the number is smaller: on both
            # seeds every entry must sit within _VERIFY_RTOL of its row
            # once _VERIFY_BOUND_UNITS of its own bound are taken off, and
            # the LARGER of the two errors counts.  A build that is off by
            # 1e-7 of a well-conditioned row fails this however small 1e-7
            # looks.
            beyond = {}
            for seed in (7, 8):
                got = compare(seed, self._rounding_floors(seed, span))
                beyond = {k: max(v, beyond.get(k, 0.0))
                          for k, v in got.items()}
            marginal = dict(raw=dict(errors), beyond_rounding_bound=beyond,
                            bound_units=self._VERIFY_BOUND_UNITS)
            logger.info('marginal disagreement %s; beyond the entries\' own '
                        'rounding-error bounds on two seeds: %s', errors,
                        beyond)
            errors = beyond
            worst = max(errors.values())
        verdict = dict(ok=bool(worst <= self._VERIFY_RTOL), referee='tape',
                       referee_version=self._REFEREE_VERSION,
                       worst=max(errors.values()), errors=errors,
                       marginal=marginal, span=list(span),
                       nodes=int(
                           min(self.num_collocation_nodes,
                               self._VERIFY_NODES)),
                       kernels={k: list(v) for k, v in hot.items()},
                       isa_exec_copies=meta.get('isa_exec_copies'),
                       isa_replaced=meta.get('isa_replaced'),
                       banned_kernels=list(meta.get('banned_kernels', ())),
                       vector_spills_in_service={
                           k: v for k, v in hb.vgpr_spills(hsaco).items()
                           if k not in meta.get('banned_kernels', ())})
        if not verdict['ok']:
            raise hb.BuildRejected(
                'kernels of %s (%s) disagree with the expression DAG '
                'evaluated by opty_hip_tape_run: %s (relative to the largest '
                'value of the equation) -- a compiler fault (DESIGN.md 4.1).'
                % (os.path.basename(hsaco), hot or 'not at the register '
                   'limit', {k: '%.3g' % v for k, v in errors.items()}),
                verdict)
        try:
            tmp = side + '.%d.tmp' % os.getpid()
            with open(tmp, 'w') as f:
                json.dump(verdict, f)
            os.replace(tmp, side)
        except OSError:
            pass
        return verdict

    _VERIFY_SPANS = ((-1.0, 1.0), (0.1, 0.9), (0.45, 0.55))

    @staticmethod
    def _row_error(got, want, row, floor=None):
        """Largest difference between two vectors relative to the largest
        (finite) reference value of the entry's own equation; ``row[k]`` =
        equation of entry ``k``.  Entries that are NaN in both, or the same
        infinity in both, agree; any other non-finite difference is inf.
        ``floor`` (array like ``want``): what an entry may differ by for
        reasons of its own conditioning -- only the excess counts."""
        if not want.size:
            return 0.0
        with np.errstate(all='ignore'):
            same = (np.isnan(got) & np.isnan(want)) | (
                np.isinf(got) & np.isinf(want) & (got == want))
            d = np.where(same, 0.0, np.abs(got - want))
            if floor is not None:
                d = np.where(d <= floor, 0.0, d)
        if not np.isfinite(d).all():
            return float('inf')
        scale = np.zeros(int(row.max()) + 1)
        np.maximum.at(scale, row, np.where(np.isfinite(want),
                                           np.abs(want), 0.0))
        scale = np.maximum(scale, 1e-300)
        return float((d/scale[row]).max())

    def _verification_inputs(self, seed=7, span=(-1.0, 1.0)):
        """``(N, free)`` of the small problem the verification evaluates:
        the first ``_VERIFY_NODES`` nodes, seeded values from ``span``."""
        N = min(self.num_collocation_nodes, self._VERIFY_NODES)
        n, q = self.num_states, self.num_unknown_input_trajectories
        rng = np.random.default_rng(seed)
        free = rng.uniform(span[0], span[1],
                           (n + q)*N + self.num_unknown_parameters
                           + int(self._variable_duration))
        if self._variable_duration:
            free[-1] = 0.01
        return N, free

    def _reference_values(self, seed=7, span=(-1.0, 1.0)):
        """Constraints and Jacobian values of the verification problem from
        the instruction tape run on the device (``opty_hip_tape_run``), in
        the layouts the kernels write: ``(con, jac, con_row, jac_row)``,
        ``*_row[k]`` = equation of entry ``k``."""
        N, free = self._verification_inputs(seed, span)
        known = self._known_trajectory_array(np.ones(self.num_free))[:, :N] \
            if self.num_known_input_trajectories else None
        return self._tape_values(free, N, 0, N - 1, known)

    def _node_inputs(self, free, N, a, b, known):
        """``inputs(kind, index)`` of the constraint nodes ``[a, b)`` of an
        ``N``-node problem: what a DAG INPUT node reads there."""
        prog = self._build_program()
        n, q = prog.n, prog.q
        tail = free[(n + q)*N:]
        kpar = [float(self.known_parameter_map[p])
                for p in self.known_parameters]

        def inputs(kind, idx):
            if kind in ('cur', 'adj'):
                src, k = prog.rows[idx]
                row = free[k*N:(k + 1)*N] if src == 'free' else known[k]
                off = prog.cur_offset if kind == 'cur' else prog.adj_offset
                return row[a + off:b + off]
            if kind == 'par':
                src, k = prog.pars[idx]
                return kpar[k] if src == 'known' else tail[k]
            assert kind == 'h', kind
            return self.node_time_interval if prog.h[0] == 'fixed' \
                else tail[prog.h[1]]
        return inputs

    def _kernel_layout(self, con_vals, jac_vals, ncn):
        """Per-root vectors of ``ncn`` nodes (``con_vals[j]``, ``jac_vals[e]``)
        in the layouts the kernels write for a node range: ``(con, jac,
        con_row, jac_row)`` with ``con[j*ncn + i]``; ``jac[i*P + e]``, or
        ``jac[S_j*ncn + i*L_j + pos]`` for the row-sorted layout;
        ``*_row[k]`` = equation of entry ``k``."""
        prog = self._build_program()
        M, P = prog.M, prog.P
        ones = np.ones(ncn)
        con = np.concatenate([np.atleast_1d(v)*ones for v in con_vals]) \
            if M else np.zeros(0)
        con_row = np.repeat(np.arange(M), ncn)
        block = np.stack([np.atleast_1d(v)*ones for v in jac_vals], axis=1) \
            if P else np.zeros((ncn, 0))                # (ncn, P)
        ent_row = np.array([j for j, _ in prog.pattern], dtype=np.int64)
        if self._jacobian_layout == 'csr':
            # jac[S_j*ncn + i*L_j + pos]
            jac = np.empty(ncn*P)
            jac_row = np.empty(ncn*P, dtype=np.int64)
            rs = prog.row_start
            for j in range(M):
                S, L = rs[j], rs[j + 1] - rs[j]
                jac[S*ncn:(S + L)*ncn] = block[:, S:S + L].ravel()
                jac_row[S*ncn:(S + L)*ncn] = j
        else:
            jac = block.ravel()
            jac_row = np.tile(ent_row, ncn)
        return con, jac, con_row, jac_row

    def _tape_values(self, free, N, a, b, known):
        """Constraints and Jacobian values of the constraint nodes ``[a, b)``
        of an ``N``-node problem with free vector ``free`` (known
        trajectories ``known``, ``(m_known, N)``), evaluated from the
        expression DAG by the instruction tape on the device
        (``opty_hip_tape_run``): ``(con, jac, con_row, jac_row)`` in the
        layouts the kernels write for that node range
        (:meth:`_kernel_layout`)."""
        from .codegen.tape import Tape
        prog = self._build_program()
        ncn = b - a
        inputs = self._node_inputs(free, N, a, b, known)
        if self._tape is None:
            self._tape = Tape(prog.dag,
                              list(prog.con_out) + list(prog.jac_out))
        tape = self._tape
        vals = hb.tape_run(tape, tape.table(ncn, inputs), self._device)
        return self._kernel_layout([vals[tape.slot[r]] for r in prog.con_out],
                                   [vals[tape.slot[r]] for r in prog.jac_out],
                                   ncn)

    #: what a kernel may differ from the tape by beyond ``_VERIFY_RTOL`` of
    #: its row: this many units of the entry's own first-order rounding-error
    #: bound (``codegen/errbound.py``; the parity tests' floor is 32 units)
    _VERIFY_BOUND_UNITS = 64.0

    def _rounding_floors(self, seed=7, span=(-1.0, 1.0)):
        """``(con_floor, jac_floor)`` in the kernels' layouts: per entry,
        ``_VERIFY_BOUND_UNITS`` x unit round-off x the running error bound of
        the entry's own operations at the verification inputs."""
        from .codegen.errbound import evaluate_with_error_bound
        prog = self._build_program()
        N, free = self._verification_inputs(seed, span)
        known = self._known_trajectory_array(np.ones(self.num_free))[:, :N] \
            if self.num_known_input_trajectories else None
        inputs = self._node_inputs(free, N, 0, N - 1, known)
        _, ce = evaluate_with_error_bound(prog.dag, list(prog.con_out),
                                          inputs)
        _, je = evaluate_with_error_bound(prog.dag, list(prog.jac_out),
                                          inputs)
        con, jac, _, _ = self._kernel_layout(ce, je, N - 1)
        unit = self._VERIFY_BOUND_UNITS*2.0**-53
        with np.errstate(all='ignore'):
            return (np.nan_to_num(con*unit, nan=0.0, posinf=0.0),
                    np.nan_to_num(jac*unit, nan=0.0, posinf=0.0))

    def _evaluate_build(self, meta, hsaco, seed=7, span=(-1.0, 1.0),
                        pattern=None, restricted=False):
        """``[con, jac, fused con, fused jac]`` of one code object of this
        problem's module on the first ``_VERIFY_NODES`` nodes: separate and
        fused launches, host buffers, no instance tails (scalar code)."""
        N, free = self._verification_inputs(seed, span)
        # every entry point launches its OWN kernel here (no plan flags, no
        # calibration: any of the three may serve a caller once the handle
        # has measured them) -- except a kernel the build banned, which no
        # entry point ever launches
        base = self._descriptor(meta)
        desc = dict(base, N=N, num_inst=0, nnz_inst=0,
                    num_inst_atoms=0, inst_folded=0, fused_loses=0,
                    jac_via_fused=0,
                    routing=base['routing'] & ~hb.ROUTE_CALIBRATE)
        if self._jacobian_layout == 'varying_first':
            desc['layout'] = 0          # the kernels write node-major blocks
        h = hb.HipProblem(desc, hsaco)
        try:
            if not self._variable_duration:
                h.set_interval(self.node_time_interval)
            if self.num_known_parameters:
                h.set_known_parameters(np.array(
                    [float(self.known_parameter_map[p])
                     for p in self.known_parameters]))
            if self.num_known_input_trajectories:
                h.set_known_trajectories(np.ascontiguousarray(
                    self._known_trajectory_array(
                        np.ones(self.num_free))[:, :N]))
            if self._program.pruned or self._jacobian_layout == 'csr':
                h.set_block_pattern(self._program.pattern)
            # Before every kernel: a known pattern into all register files
            # (``pattern``; default NaNs).  The three kernels evaluate the
            # same expressions of the same inputs one after the other, so a
            # kernel that reads a register it never wrote (two of the frozen
            # hipcc faults do) may find the RIGHT value there, left by its
            # predecessor -- a box of r05 accepted
            # tools/o3_repro/one_legged_park_spill_O2 that way.  Every output
            # is a device vector of its own that starts as NaNs: a store that
            # never happens shows.  (Through host arrays the fused kernel's
            # values passed through the handle's buffers, where opty_jac's
            # were still lying: tools/o3_repro/biped_csr_persistent_O2, a
            # fused kernel that drops stores, was accepted that way.)
            pattern = hb.POISON if pattern is None else pattern
            ncon, nnz = self.num_eom*(N - 1), h.nnz
            dfree = hb.DeviceVector(free, self._device)
            outs = [hb.DeviceVector(np.full(n, np.nan), self._device)
                    for n in (ncon, nnz, ncon, nnz)]
            hb.poison_registers(pattern)
            h.eval_con(dfree, outs[0], hb.DEVICE)
            h.synchronize()
            hb.poison_registers(pattern)
            h.eval_jac(dfree, outs[1], hb.DEVICE)
            h.synchronize()
            hb.poison_registers(pattern)
            h.eval_con_jac(dfree, outs[2], outs[3], hb.DEVICE)
            h.synchronize()
            if restricted:
                # ``[..., jac (opty_jac_var), con, jac (opty_conjac_var)]``
                # as well: registered outputs, written whole for another
                # seed's free vector first, then by the restricted kernels
                other = hb.DeviceVector(
                    self._verification_inputs(seed + 1000, span)[1],
                    self._device)
                outs += [hb.DeviceVector(np.full(n, np.nan), self._device)
                         for n in (nnz, ncon, nnz)]
                for jac in (outs[4], outs[6]):
                    h.output_register(jac)
                h.eval_jac(other, outs[4], hb.DEVICE)
                h.eval_con_jac(other, outs[5], outs[6], hb.DEVICE)
                h.synchronize()
                hb.poison_registers(pattern)
                h.eval_jac(dfree, outs[4], hb.DEVICE)
                h.synchronize()
                if h.routing()['flavour'] != 'restricted' and os.environ.get(
                        'OPTY_HIP_DENSE_OUTPUT', '0') in ('', '0'):
                    raise hb.HipBackendError(
                        'the restricted Jacobian kernel did not serve a '
                        'registered output')
                hb.poison_registers(pattern)
                h.eval_con_jac(dfree, outs[5], outs[6], hb.DEVICE)
                h.synchronize()
                other.close()
            vals = [o.numpy() for o in outs]
            for o in outs + [dfree]:
                o.close()
            return vals
        finally:
            h.close()

    def tune_launch(self, **kwargs):
        """Times the neighbouring launch geometries of this problem on the
        device, records the winners in the launch-plan file
        (:mod:`opty_amd.launch_plan`) and rebuilds this collocator's kernels
        with them.  Returns the plan entry."""
        from . import launch_plan
        entry = launch_plan.tune(self, **kwargs)
        if self._hip is not None:
            self._hip.close()
        self._hip = None
        if kwargs.get('save', True):
            # the recorded plan is what the next build looks up; options the
            # caller fixed stay in force when nothing was recorded
            self._emit_options = None
        return entry

    def cross_check(self, free=None, window=4096, opt_level='-O1',
                    referee='tape'):
        """Evaluates this problem's kernels on ``free`` (default: seeded
        random values) over the first and last ``window`` constraint nodes
        and returns their largest disagreement with a referee:

        * ``referee='tape'`` (node-major layouts): the expression DAG itself,
          executed as an instruction tape on the device
          (``opty_hip_tape_run``) -- the error of the
          build in use, each entry relative to the largest value of its
          equation in the window (rounding level, ~1e-15, for a right build);
          the window is capped so that the tape's value table stays below
          512 MB;
        * ``referee='-O1'`` (and the row-sorted layout): a build of the SAME
          generated module that went through another compiler pipeline
          (``hipcc`` with ``opt_level``), relative to the largest value of
          each vector.  A disagreement then means that ONE of the two builds
          is faulty, not which: round 4 met ``-O1`` kernels that were the
          wrong ones.

        Builds at the register limit go through the tape check on 131 seeded
        nodes before their handle exists (:meth:`_verify_build`); this is the
        same comparison on demand, over larger node windows and with the
        caller's ``free``.  Needs ``torch``."""
        if referee == 'tape' and self._jacobian_layout == 'coo':
            return self._cross_check_tape(free, window)
        import torch
        hip = self._ensure_hip()
        meta = self._kernel_meta
        hsaco = self._compile(self._built_source, opt_level=opt_level)
        twin = hb.HipProblem(self._descriptor(meta), hsaco)
        try:
            self._install_tables(twin)
            if free is None:
                free = np.random.default_rng(7).uniform(-1.0, 1.0,
                                                        self.num_free)
                if self._variable_duration:
                    free[-1] = 0.01
            free = self._host_free(free)
            self._sync_known(hip, free)
            self._uploaded_parameters = self._uploaded_trajectories = None
            self._sync_known(twin, free)
            if self._jacobian_layout != 'coo':
                # the row-sorted layout is not evaluated by node ranges
                outs = []
                for h in (hip, twin):
                    con = np.empty(self.num_constraints)
                    jac = np.empty(h.nnz)
                    h.eval_con_jac(free, con, jac, hb.HOST)
                    outs.append((con, jac))
                return max(float(np.abs(x - y).max()) /
                           max(float(np.abs(x).max()), 1e-300)
                           for x, y in zip(*outs))
            dev = torch.device('cuda', self._device)
            ncn = self.num_collocation_nodes - 1
            w = max(1, min(int(window), ncn))
            windows = sorted({(0, w), (ncn - w, ncn)})
            P, M = self._program.P, self.num_eom
            d_free = torch.from_numpy(free).to(dev)
            worst = 0.0
            for a, b in windows:
                outs = []
                for h in (hip, twin):
                    con = torch.empty((M, b - a), dtype=torch.float64,
                                      device=dev)
                    jac = torch.empty((b - a)*P, dtype=torch.float64,
                                      device=dev)
                    h.eval_shard(hb.EVAL_FUSED, d_free, con, b - a, jac, a, b)
                    h.synchronize()
                    outs.append((con.cpu().numpy(), jac.cpu().numpy()))
                for x, y in zip(*outs):
                    scale = max(float(np.abs(x).max()), 1e-300)
                    worst = max(worst, float(np.abs(x - y).max())/scale)
            return worst
        finally:
            twin.close()
            # the upload cache belongs to the handle in use
            self._uploaded_parameters = self._uploaded_trajectories = None

    def _cross_check_tape(self, free, window):
        import torch
        hip = self._ensure_hip()
        if free is None:
            free = np.random.default_rng(7).uniform(-1.0, 1.0, self.num_free)
            if self._variable_duration:
                free[-1] = 0.01
        free = self._host_free(free)
        self._sync_known(hip, free)
        prog = self._build_program()
        N = self.num_collocation_nodes
        ncn = N - 1
        known = self._known_trajectory_array(free) \
            if self.num_known_input_trajectories else None
        from .codegen.tape import Tape
        if self._tape is None:
            self._tape = Tape(prog.dag,
                              list(prog.con_out) + list(prog.jac_out))
        cap = max(64, (512 << 20)//(8*max(1, self._tape.nslots)))
        w = max(1, min(int(window), ncn, cap))
        dev = torch.device('cuda', self._device)
        d_free = torch.from_numpy(free).to(dev)
        P, M = prog.P, self.num_eom
        worst = 0.0
        for a, b in sorted({(0, w), (ncn - w, ncn)}):
            con = torch.empty((M, b - a), dtype=torch.float64, device=dev)
            jac = torch.empty((b - a)*P, dtype=torch.float64, device=dev)
            hip.eval_shard(hb.EVAL_FUSED, d_free, con, b - a, jac, a, b)
            hip.synchronize()
            rcon, rjac, con_row, jac_row = self._tape_values(free, N, a, b,
                                                             known)
            worst = max(worst,
                        self._row_error(con.cpu().numpy().ravel(), rcon,
                                        con_row),
                        self._row_error(jac.cpu().numpy(), rjac, jac_row))
        return worst

    def _descriptor(self, meta):
        prog = self._build_program()
        return dict(
            N=self.num_collocation_nodes, n=self.num_states, M=self.num_eom,
            m_known=self.num_known_input_trajectories,
            q=self.num_unknown_input_trajectories,
            p_known=self.num_known_parameters,
            r=self.num_unknown_parameters, s=int(self._variable_duration),
            C=prog.C, P=prog.P,
            method=0 if self.integration_method == 'backward euler' else 1,
            num_inst=self.num_instance_constraints,
            nnz_inst=len(self._inst_rows),
            num_inst_atoms=len(self._inst_atoms),
            jac_wgs_per_block=meta['kernels']['jac']['wgs_per_block'],
            jac_waves_per_wg=meta['kernels']['jac']['waves_per_wg'],
            fused_wgs_per_block=meta['kernels']['conjac']['wgs_per_block'],
            con_wgs_per_block=meta['kernels']['con']['wgs_per_block'],
            fused_waves_per_wg=meta['kernels']['conjac']['waves_per_wg'],
            con_waves_per_wg=meta['kernels']['con']['waves_per_wg'],
            num_uniform=meta['num_uniform'],
            uniform_dynamic=int(meta['uniform_dynamic']),
            device=self._device,
            layout={'coo': 0, 'csr': 1,
                    'varying_first': 2}[self._jacobian_layout],
            inst_folded=int(meta.get('inst_folded', False)),
            fused_loses=self._fused_loses(),
            jac_via_fused=self._plan_flag('jac_via_fused'),
            routing=self._routing_bits(meta),
            jac_persist=meta['kernels']['jac'].get('persist', 0),
            fused_persist=meta['kernels']['conjac'].get('persist', 0),
            jac_class_cost=self._class_cost(meta, 'jac'),
            fused_class_cost=self._class_cost(meta, 'conjac'),
            **self._restricted_geometry(meta))

    def _restricted_geometry(self, meta):
        """``opty_hip_desc.var_*``: zeros unless the module carries the
        restricted kernels and the build accepted them."""
        ok = meta.get('restricted_ok') is True and \
            self._jacobian_layout == 'coo'
        jv, fv = (meta['kernels'][k] for k in ('jac_var', 'conjac_var')) \
            if ok else ({}, {})
        geo = dict(
            var_jac_wgs_per_block=jv.get('wgs_per_block', 0),
            var_jac_waves_per_wg=jv.get('waves_per_wg', 0),
            var_fused_wgs_per_block=fv.get('wgs_per_block', 0),
            var_fused_waves_per_wg=fv.get('waves_per_wg', 0))
        if ok and meta.get('run_hsaco'):
            # run form (EmitOptions.var_order): what the handle passes to
            # opty_hip_set_restricted_runs
            jr, fr = (meta['run']['kernels'][k]
                      for k in ('jac_var', 'conjac_var'))
            geo.update(
                var_run_code_object=meta['run_hsaco'],
                var_jac_persist=jr['run_persist'],
                var_fused_persist=fr['run_persist'],
                var_jac_class_cost=tuple(float(c) for c in jr['class_cost']),
                var_fused_class_cost=tuple(
                    float(c) for c in fr['class_cost']))
        return geo

    def _routing_bits(self, meta):
        """``opty_hip_desc.routing``: the handle calibrates which kernels
        serve ``EVAL_FUSED`` / ``EVAL_JAC`` on its own device (the plan's
        ``fused_pays`` / ``jac_via_fused`` break ties; ``OPTY_HIP_ROUTING=
        plan`` keeps them as they are), and never launches a kernel the
        build marked unusable (``meta['banned_kernels']``)."""
        bits = hb.ROUTE_CALIBRATE
        banned = meta.get('banned_kernels', ())
        if 'opty_jac' in banned:
            bits |= hb.ROUTE_NO_JAC_KERNEL
        if 'opty_conjac' in banned:
            bits |= hb.ROUTE_NO_FUSED_KERNEL
        return bits

    def _class_cost(self, meta, key):
        """Relative wave durations of a persistent kernel's strip classes
        (``opty_hip_desc.*_class_cost``): measured ones from the launch plan
        (``"jac_durations"`` / ``"fused_durations"``, recorded by the tuner
        from a traced launch) when they fit the kernel, else the printer's
        estimate."""
        k = meta['kernels'][key]
        if not k.get('persist'):
            return ()
        cost = list(k['class_cost'])
        if self._emit_options is None:
            from . import launch_plan
            entry = launch_plan.lookup_entry(self._build_program(),
                                             self._launch_blocks()) or {}
            got = entry.get('fused_durations' if key == 'conjac'
                            else 'jac_durations')
            if got and len(got) == len(cost):
                cost = list(got)
        return tuple(float(c) for c in cost)

    def _fused_loses(self):
        """1 when the launch plan of this problem and launch size measured
        the fused kernel slower than ``opty_con`` + ``opty_jac`` (``"fused_
        pays": false``): ``opty_hip_eval_con_jac`` / ``EVAL_FUSED`` then issue
        those two launches."""
        if self._emit_options is not None:
            return 0
        from . import launch_plan
        entry = launch_plan.lookup_entry(self._build_program(),
                                         self._launch_blocks())
        return int(bool(entry) and entry.get('fused_pays') is False)

    def _plan_flag(self, tag):
        """1 when the launch plan of this problem and launch size says
        ``tag`` (``"jac_via_fused": true``: ``EVAL_JAC`` launches the fused
        kernel, measured faster than ``opty_jac``)."""
        if self._emit_options is not None or \
                self._jacobian_layout != 'coo':
            return 0
        from . import launch_plan
        entry = launch_plan.lookup_entry(self._build_program(),
                                         self._launch_blocks())
        return int(bool(entry) and entry.get(tag) is True)

    def _known_trajectory_array(self, free):
        vals = []
        for f in self.known_input_trajectories:
            v = self.known_trajectory_map[f]
            vals.append(v(free) if callable(v) else v)
        return np.array(vals, dtype=np.float64)

    def _ensure_hip(self):
        """Builds (or fetches from the cache) the code object, creates the
        device handle and uploads the node-invariant data."""
        if self._hip is not None:
            return self._hip
        logger.info('Compiling the HIP constraint/Jacobian kernels.')
        hsaco, meta = self._verified_code_object()
        hip = hb.HipProblem(self._descriptor(meta), hsaco)
        hip.literals = self._known_scalars() if self._specialize else None
        self._install_tables(hip)
        self._kernel_meta = meta
        self._hip = hip
        for jac, a, b in getattr(self, '_owned_outputs', ()):
            hip.output_register(jac, a, b)
        return hip

    def _verified_code_object(self):
        """``(hsaco, meta)`` of the build the referee accepts -- the verdict
        is in ``_build_verdict``: :meth:`_build_code_object`'s, or, when it
        is refused and the caller did not fix the geometry, a neighbouring
        one (:meth:`_verified_alternative`)."""
        hsaco, meta = self._build_code_object()
        try:
            meta, self._build_verdict = self._verify_with_run_form(hsaco,
                                                                   meta)
        except hb.BuildRejected as err:
            if self._emit_options is not None or self._pinned is not None:
                raise               # the caller fixed the geometry
            hsaco, meta, self._build_verdict = self._verified_alternative(
                hsaco, meta, err)
        return hsaco, meta

    def _verify_with_run_form(self, hsaco, meta):
        """``(meta, verdict)`` of :meth:`_verify_build`.  A build that the
        referee refuses while it carries the run form of the restricted
        kernels is judged again without it (``meta['run_hsaco']`` None: the
        module's dispatch form serves): the form is an extra, like the
        restricted kernels themselves."""
        try:
            return meta, self._verify_build(hsaco, meta)
        except hb.BuildRejected as err:
            if not meta.get('run_hsaco'):
                raise
            logger.info('the run form of the restricted kernels of %s is '
                        'not used (refused by the referee)',
                        os.path.basename(hsaco))
            self._run_form_refused = 'referee: %s' % (str(err)[:300],)
            meta = dict(meta, run_hsaco=None)
            return meta, self._verify_build(hsaco, meta)

    def _register_output(self, jac, node_begin, node_end):
        """``HipProblem.output_register`` for a device Jacobian buffer the
        caller owns for this collocator's lifetime -- now, or as soon as
        the handle exists (it is built lazily)."""
        if not hasattr(self, '_owned_outputs'):
            self._owned_outputs = []
        self._owned_outputs.append((jac, node_begin, node_end))
        if self._hip is not None:
            self._hip.output_register(jac, node_begin, node_end)

    def _unregister_output(self, jac):
        owned = getattr(self, '_owned_outputs', [])
        keep = [o for o in owned if o[0] is not jac]
        if len(keep) != len(owned):
            self._owned_outputs = keep
            if self._hip is not None and getattr(self._hip, '_h', None):
                self._hip.output_unregister(jac)

    def _respecialize(self, hip):
        self._literal_values = None
        hsaco, meta = self._verified_code_object()
        hip.reload(self._descriptor(meta), hsaco)
        hip.literals = self._known_scalars() if self._specialize else None
        self._kernel_meta = meta
        self._uploaded_parameters = self._uploaded_trajectories = None
        self._install_tables(hip)

    def _install_tables(self, hip):
        """Uploads the node-invariant data of this problem into a handle."""
        if not self._variable_duration:
            hip.set_interval(self.node_time_interval)
        self._callable_known = any(
            callable(v) for v in self.known_trajectory_map.values())
        self._uploaded_parameters = self._uploaded_trajectories = None
        self._sync_known(hip, None)
        if self._callable_known and self.num_known_input_trajectories:
            # placeholders until the first evaluation supplies `free`
            hip.set_known_trajectories(self._known_trajectory_array(
                np.ones(self.num_free)))
            self._uploaded_trajectories = None
        if self._program.pruned or self._jacobian_layout == 'csr':
            hip.set_block_pattern(self._program.pattern)
        if self._jacobian_layout == 'varying_first':
            order, seg_len, source = self.jacobian_segments()
            hip.set_segments(order, seg_len, source)
        if self._jacobian_layout == 'coo':
            # entries that repeat another varying entry's expression are
            # filled on the host (OPTY_HOST_NO_COPIES=1: moved like the rest)
            self._install_copies(hip)
        if self.num_instance_constraints:
            idx = self.instance_constraints_free_index_map
            hip.set_instance_indices([idx[f] for f in self._inst_atoms],
                                     self._inst_rows, self._inst_cols)

    def _install_copies(self, hip):
        """Tells the handle which block entries the host path moves and which
        it fills from another entry of the same block: exact duplicates, and
        (r06) node-invariant multiples of a moved entry, with factors
        evaluated here from the CURRENT known parameters / fixed interval
        (``codegen.program.scaled_copies``; set again by :meth:`_sync_known`
        when those change).  ``OPTY_HOST_NO_COPIES=1``: every varying entry
        is moved; ``=exact``: exact duplicates only (A/B runs)."""
        from .codegen.program import scaled_copies, chain_value
        from .codegen.evaluate import evaluate_uniform
        prog = self._program
        mode = os.environ.get('OPTY_HOST_NO_COPIES', '')
        unique, copies = varying_copies(prog)
        self._copy_chains = None
        if mode == '1':
            hip.set_varying_entries(sorted(unique + [d for d, _ in copies]))
            hip.set_entry_copies([])
            return
        if mode != 'exact':
            u2, c2 = scaled_copies(prog)
            scales = self._copy_scales(c2)
            if scales is not None:
                hip.set_varying_entries(u2)
                hip.set_entry_copies(c2, scales)
                self._copy_chains = c2
                self._copy_scale_values = scales
                return
        hip.set_varying_entries(unique)
        hip.set_entry_copies(copies)

    def _copy_scales(self, chains):
        """Factors of the scaled copies for the current known values, or
        None when one of them is not a finite non-zero number (the caller
        then moves those entries instead)."""
        from .codegen.program import chain_value
        from .codegen.evaluate import evaluate_uniform
        prog = self._program
        par, h = self._known_scalars()

        def scalar(kind, idx):
            if kind == 'par':
                src, k = prog.pars[idx]
                return par[k] if src == 'known' else None
            if kind == 'h':
                return h if prog.h[0] == 'fixed' else None
            return None

        nodes = sorted({st[1] for c in chains for ch in (c[2], c[3])
                        for st in ch if len(st) > 1})
        try:
            vals = evaluate_uniform(prog.dag, nodes, scalar)
        except (ArithmeticError, ValueError):
            return None
        if any(n not in vals for n in nodes):
            return None
        out = []
        for dst, src, num, den in chains:
            if num == den:
                out.append(1.0)         # the same expression: bit for bit
                continue
            try:
                d = chain_value(den, vals)
                v = chain_value(num, vals)/d
            except ZeroDivisionError:
                return None
            if not (np.isfinite(v) and np.isfinite(d) and d != 0.0):
                return None
            out.append(float(v))
        return np.array(out, dtype=np.float64)

    @property
    def hip(self):
        """The :class:`opty_amd.hip_backend.HipProblem` handle (device-pointer
        evaluation, timing)."""
        return self._ensure_hip()

    def _sync_known(self, hip, free):
        """Brings the device copies of the known parameters and trajectories
        up to date with ``known_parameter_map`` / ``known_trajectory_map``.

        The reference reads both maps on every call (``_merge_fixed_free``,
        ``opty/direct_collocation.py:2891-2926``), so a user may change a
        value between solves (``plot_human_gait.py`` does:
        ``prob.collocator.known_parameter_map[g] = ...``).  Here the maps are
        re-read on every call too, compared with what the device holds and
        re-uploaded only when they differ.  Known trajectories given as
        functions of ``free`` (``:2916-2917``) are re-evaluated on the host
        every call; ``free`` is None at setup, when those are skipped."""
        if self._specialize and hip is self._hip and \
                self._specialized_for is not None and \
                self._known_scalars() != self._specialized_for:
            # the kernels carry the OLD values as literals: print, compile
            # and verify them again for the new ones, inside the same handle
            # object (closures hold on to it)
            self._respecializations += 1
            if self._auto_specialized and self._respecializations >= 2:
                # automatic specialisation is for solves with FIXED
                # parameters: this caller's keep changing
                logger.warning('known parameters changed again: back to the '
                               'generic kernels (specialize_parameters=True '
                               'keeps rebuilding instead)')
                self._specialize = False
                self._auto_specialized = None      # never again
                self._literal_values = self._specialized_for = None
            else:
                logger.warning('known parameters changed: rebuilding the '
                               'parameter-specialised kernels')
            self._respecialize(hip)
        if self.num_known_parameters:
            vals = np.array([float(self.known_parameter_map[p])
                             for p in self.known_parameters])
            if (self._uploaded_parameters is None or
                    not np.array_equal(vals, self._uploaded_parameters)):
                hip.set_known_parameters(vals)
                stale = self._uploaded_parameters is not None
                self._uploaded_parameters = vals
                if stale and hip is self._hip and \
                        getattr(self, '_copy_chains', None):
                    # the host path's scaled copies carry factors of the
                    # old values
                    self._install_copies(hip)
        if self.num_known_input_trajectories:
            if self._callable_known and free is None:
                return
            vals = self._known_trajectory_array(free)
            if vals.shape != (self.num_known_input_trajectories,
                              self.num_collocation_nodes):
                raise ValueError('every known trajectory must have {} '
                                 'values.'.format(self.num_collocation_nodes))
            if (self._uploaded_trajectories is None or
                    not np.array_equal(vals, self._uploaded_trajectories)):
                hip.set_known_trajectories(vals)
                # np.array above copied: later in-place edits of the user's
                # arrays are seen as a difference
                self._uploaded_trajectories = vals

    @staticmethod
    def _merge_fixed_free(syms, fixed, free, typ, free_op_vals):
        """The known (``fixed``: symbol -> float, array or callable of the
        free vector ``free_op_vals``) and the unknown (``free``: ``(r,)``,
        ``(N,)`` or ``(q, N)``) values of ``syms`` interleaved in ``syms``
        order; ``typ`` is ``'par'`` or ``'traj'`` -- the reference's static
        helper with its signature (``opty/direct_collocation.py:2891-2926``).
        The evaluation path does not call it: the kernels read the known
        tables and ``free`` directly, :meth:`_sync_known` keeps the tables
        current."""
        merged, taken = [], 0
        for s in syms:
            if s in fixed:
                v = fixed[s]
                merged.append(v(free_op_vals) if callable(v) else v)
            elif typ == 'traj' and np.ndim(free) == 1:
                merged.append(free)
            else:
                merged.append(free[taken])
                taken += 1
        return np.array(merged)

    def sync_known(self):
        """Uploads changed ``known_parameter_map`` / ``known_trajectory_map``
        values now; for callers that evaluate through :attr:`hip` with device
        pointers (the host callbacks do this on every call)."""
        self._sync_known(self._ensure_hip(), None)

    # ------------------------------------------------------------------
    # the reference's multi-argument closures, on the plugin call shape
    # (opty/direct_collocation.py:2304-2446, :2692-2887)
    # ------------------------------------------------------------------
    def _multi_arg_dag(self):
        """The discretised equations lowered over the reference's argument
        list ``x_i(n), x_p|x_n(n), s_i(m)[, s_n(m)], parameters(p), h``
        (``:2347-2359``): vector argument ``k`` is DAG input ``('cur', k)``,
        the ``p + 1`` trailing scalars are the const arguments."""
        from .codegen import ir
        from .codegen.lower import Lowerer
        be = self.integration_method == 'backward euler'
        vec = (self.current_discrete_state_symbols +
               (self.previous_discrete_state_symbols if be
                else self.next_discrete_state_symbols) +
               self.current_discrete_specified_symbols)
        if not be:
            vec += self.next_discrete_specified_symbols
        const = self.parameters + (self.time_interval_symbol,)
        dag = ir.DAG()
        table = {s: dag.input('cur', k) for k, s in enumerate(vec)}
        table.update({s: dag.input('par', k) for k, s in enumerate(const)})
        low = Lowerer(dag, table)
        con = [low.lower(e) for e in self.discrete_eom]
        # r_i(x_i): d/dx_i through the argument that carries dr/dx
        n, m = self.num_states, self.num_input_trajectories
        chain = {}
        for k, st, kd in self._implicit_chain():
            chain[dag.input('cur', 2*n + k)] = [
                (dag.input('cur', st), dag.input('cur', 2*n + kd))]
            if not be:
                chain[dag.input('cur', 2*n + m + k)] = [
                    (dag.input('cur', n + st),
                     dag.input('cur', 2*n + m + kd))]
        return dag, table, con, len(vec), len(const), chain

    def _multi_arg_values(self, state_values, specified_values,
                          constant_values, interval_value):
        """The reference closures' slicing of their four arguments into the
        compiled function's argument list (``:2408-2437``, ``:2866-2887``)."""
        N = self.num_collocation_nodes
        assert state_values.shape == (self.num_states, N)
        be = self.integration_method == 'backward euler'
        cur = slice(1, None) if be else slice(None, -1)
        adj = slice(None, -1) if be else slice(1, None)
        args = [x for x in state_values[:, cur]]
        args += [x for x in state_values[:, adj]]
        specified_values = np.asarray(specified_values)
        if specified_values.ndim == 2:
            assert specified_values.shape == (self.num_input_trajectories, N)
            args += [u for u in specified_values[:, cur]]
            if not be:
                args += [u for u in specified_values[:, adj]]
        elif specified_values.ndim == 1 and specified_values.size != 0:
            assert specified_values.shape == (N,)
            args += [specified_values[cur]]
            if not be:
                args += [specified_values[adj]]
        args = [np.ascontiguousarray(a, dtype=np.float64) for a in args]
        return args + [float(c) for c in constant_values] + \
            [float(interval_value)]

    def _gen_multi_arg_con_func(self):
        """Instantiates ``_multi_arg_con_func(state_values (n, N),
        specified_values (m, N) or (N,), constant_values (p,),
        interval_value) -> (M*(N-1),)``, equation-major, on top of the
        plugin call shape ``f(result, *args)`` (:func:`opty_amd.utils.
        ufuncify_matrix`) -- ``opty/direct_collocation.py:2304-2446``.  The
        fused path (:meth:`generate_constraint_function`) does not go through
        this."""
        from .utils import _MatrixFunction
        dag, _, con, nvec, nconst, _ = self._multi_arg_dag()
        f = _MatrixFunction(dag, con, nvec, range(nvec, nvec + nconst),
                            nvec + nconst, (self.num_eom, 1), self.tmp_dir,
                            self.show_compile_output, self._device)

        def constraints(state_values, specified_values, constant_values,
                        interval_value):
            args = self._multi_arg_values(state_values, specified_values,
                                          constant_values, interval_value)
            result = np.empty((self.num_collocation_nodes - 1, self.num_eom))
            return f(result, *args).T.flatten()

        self._multi_arg_con_func = constraints

    def _gen_multi_arg_con_jac_func(self):
        """Instantiates ``_multi_arg_con_jac_func(...) -> ((N-1)*M*C,)``:
        the dense per-node blocks, node-major, in ``jacobian_indices()``
        order (``opty/direct_collocation.py:2692-2887``)."""
        from .utils import _MatrixFunction
        from .codegen.lower import forward_jacobian
        dag, table, con, nvec, nconst, chain = self._multi_arg_dag()
        jac = forward_jacobian(dag, con, [table[s] for s in self._wrt()],
                               chain)
        C = len(self._wrt())
        f = _MatrixFunction(dag, [node for row in jac for node in row], nvec,
                            range(nvec, nvec + nconst), nvec + nconst,
                            (self.num_eom, C), self.tmp_dir,
                            self.show_compile_output, self._device)
        result = np.empty((self.num_collocation_nodes - 1, self.num_eom*C))

        def constraints_jacobian(state_values, specified_values,
                                 parameter_values, interval_value):
            args = self._multi_arg_values(state_values, specified_values,
                                          parameter_values, interval_value)
            return f(result, *args).ravel()

        self._multi_arg_con_jac_func = constraints_jacobian

    def _host_free(self, free):
        return host_vector(free, 'free', self.num_free)

    def _sync_free(self, free):
        """:meth:`_sync_known` for a converted ``free``, a host array or a
        tensor (known trajectories given as functions of ``free`` are host
        callables: they alone need a device ``free`` on the host)."""
        if on_device(free):
            free = free.cpu().numpy() if self._callable_known else None
        self._sync_known(self._hip, free)

    # ------------------------------------------------------------------
    # public evaluation API (opty/direct_collocation.py:3003-3015, :2450)
    # ------------------------------------------------------------------
    def generate_constraint_function(self, recycle=False):
        """Returns ``f(free) -> ndarray (M*(N-1) + o,)``: the constraints,
        equation-major, followed by the instance constraints -- a fresh array
        per call, as in the reference (``:2444``).

        ``recycle=True`` (what :class:`Problem` asks for: cyipopt copies the
        result before the next callback): the results live in up to four
        page-locked arrays -- the kernels of small problems write into them
        directly, large ones come down by DMA without the runtime's staging;
        page-locking costs far more than an evaluation -- and one of them is
        handed out again when no Python object refers to it any more (the
        array or a view of it: NumPy views keep their base alive).  That
        test is CPython's reference count; a holder that keeps only a raw
        pointer (``ctypes``, a C extension) is invisible to it, which is why
        recycling is opt-in, and it is never done on interpreters without
        reference counts or without the GIL."""
        logger.info('Generating constraint function.')
        hip = self._ensure_hip()
        import sys
        counted = (recycle and sys.implementation.name == 'cpython' and
                   hasattr(sys, 'getrefcount') and
                   getattr(sys, '_is_gil_enabled', lambda: True)())
        ring = []
        n = self.num_constraints

        def fresh():
            if not counted:
                return np.empty(n)
            for k in range(len(ring)):
                if sys.getrefcount(ring[k]) == 2:   # the ring + this probe
                    return ring[k]
            if len(ring) < 4:
                ring.append(hb.pinned_empty(n))
                return ring[-1]
            # a caller that keeps many results alive gets pageable arrays,
            # as from the reference: page-locked memory is not for hoarding
            return np.empty(n)

        def constraints(free):
            free = self._host_free(free)
            self._sync_known(hip, free)
            out = fresh()
            hip.eval_con(free, out, hb.HOST)
            return out
        return constraints

    def generate_jacobian_function(self):
        """Returns ``f(free) -> ndarray (M*C*(N-1) + nnz_inst,)``: the dense
        per-node blocks, node-major, followed by the instance partials.  The
        returned array is a persistent buffer that the next call overwrites
        (as in the reference, ``:2814``, ``:2887``)."""
        logger.info('Generating jacobian function.')
        hip = self._ensure_hip()
        # page-locked: the (up to GB-sized) copy back runs at PCIe rate
        result = hb.pinned_empty(hip.nnz)
        # Large blocks: after the first call only the entries that can change
        # cross PCIe (opty_hip_eval_jac_persistent; the node-invariant ones
        # stay in `result`, which the caller must therefore treat as
        # read-only -- cyipopt copies it).  OPTY_HOST_DENSE=1 moves the whole
        # vector every call.
        import os
        persistent = (self._jacobian_layout == 'varying_first' or
                      self._jacobian_layout == 'coo' and
                      hip.nnz >= self._PERSISTENT_MIN_NNZ and
                      os.environ.get('OPTY_HOST_DENSE') != '1')

        # `result` is a new allocation: whatever the handle last filled at
        # this address (a dropped closure's buffer can come back from the
        # allocator) is not in it
        state = {'fresh': True}

        def jacobian(free):
            free = self._host_free(free)
            self._sync_known(hip, free)
            if persistent:
                hip.eval_jac_persistent(free, result, state['fresh'])
                state['fresh'] = False
            else:
                hip.eval_jac(free, result, hb.HOST)
            return result
        return jacobian

    #: Jacobian values below which the whole vector is copied every call (one
    #: DMA of a few MB beats a pack kernel + chunks + host threads)
    _PERSISTENT_MIN_NNZ = 1 << 20

    def jacobian_indices(self):
        """Row and column indices (int64) of every Jacobian value, in the
        order ``generate_jacobian_function`` returns them."""
        hip = self._ensure_hip()
        rows = np.empty(hip.nnz, dtype=np.int64)
        cols = np.empty(hip.nnz, dtype=np.int64)
        hip.jacobian_indices(rows, cols, hb.HOST)
        return rows, cols

    def jacobian_segments(self):
        """``(order, seg_len, copy_source)`` of ``jacobian_layout=
        'varying_first'``: ``order[pos]`` = the reference's block entry
        ``e = j*C + k`` stored at position ``pos`` of a node's block,
        ``seg_len`` = lengths of the three segments -- entries that can
        differ between two evaluations / entries that are the same
        expression as one of those (``copy_source[k]``: the position of the
        source in segment 0) / entries that depend on known parameters and
        the node time interval alone.  ``jacobian(free)`` is
        ``[seg 0 of all nodes | seg 1 of all nodes | seg 2 of all nodes |
        instance partials]``, each segment node-major."""
        prog = self._build_program()
        unique, copies = varying_copies(prog)
        taken = set(unique) | {d for d, _ in copies}
        invariant = [e for e in range(prog.P) if e not in taken]
        place = {e: k for k, e in enumerate(unique)}
        order = list(unique) + [d for d, _ in copies] + invariant
        return (np.array(order, dtype=np.int32),
                np.array([len(unique), len(copies), len(invariant)],
                         dtype=np.int32),
                np.array([place[src] for _, src in copies], dtype=np.int32))

    def jacobian_csr_structure(self):
        """``(row_ptr, col_idx)`` (int64) of the constraint Jacobian in
        compressed-sparse-row form, for ``jacobian_layout='csr'``: the values
        ``generate_jacobian_function`` returns are then ``data`` of
        ``scipy.sparse.csr_matrix((data, col_idx, row_ptr))`` as they are.
        Rows are the reference's constraint order (``j*(N-1) + i``, then the
        instance constraints), columns ascend within a row."""
        if self._jacobian_layout != 'csr':
            raise ValueError("jacobian_csr_structure needs "
                             "jacobian_layout='csr'.")
        prog = self._build_program()
        ncn = self.num_collocation_nodes - 1
        rs = np.asarray(prog.row_start, dtype=np.int64)
        lens = np.diff(rs)
        # row j*(N-1) + i starts at S_j*(N-1) + i*L_j
        starts = (rs[:-1, None]*ncn +
                  np.arange(ncn, dtype=np.int64)[None, :]*lens[:, None])
        row_ptr = np.empty(self.num_constraints + 1, dtype=np.int64)
        row_ptr[:self.num_eom*ncn] = starts.ravel()
        base = prog.P*ncn
        counts = np.bincount(self._inst_rows - self.num_eom*ncn,
                             minlength=self.num_instance_constraints) \
            if self.num_instance_constraints else np.zeros(0, dtype=np.int64)
        row_ptr[self.num_eom*ncn:] = base + np.concatenate(
            ([0], np.cumsum(counts)))
        _, cols = self.jacobian_indices()
        return row_ptr, cols

    # host helpers with the reference's names ---------------------------
    def eval_instance_constraints(self, free):
        con = self.generate_constraint_function()(free)
        return con[self.num_eom*(self.num_collocation_nodes - 1):]

    def eval_instance_constraints_jacobian_values(self, free):
        jac = self.generate_jacobian_function()(free)
        return jac[len(jac) - len(self._inst_rows):].copy()


class Problem(object):
    """NLP facade with the reference's constructor and callbacks
    (``opty/direct_collocation.py:139-145``, ``:442-567``).

    The reference subclasses ``cyipopt.Problem``; ``cyipopt`` is imported
    lazily here so that the collocator, the callbacks and the bounds arrays
    work without IPOPT.  ``solve`` needs ``cyipopt``.  Extra keywords
    ``device``, ``prune_zeros``, ``jacobian_layout``, ``deterministic``,
    ``verify_builds`` and ``specialize_parameters`` go to the collocator;
    ``jacobianstructure()`` always matches what ``jacobian(free)`` returns.

    ``prune_zeros=True`` is the recommended setting when IPOPT runs on the
    host: the callbacks move the Jacobian values over PCIe on every call
    (14.4 ms for the 792 MB of the 10-link pendulum at N = 100 000, 100x the
    kernel), the structure only once, and IPOPT does not need the structural
    zeros the reference hands over (38.6 M instead of 99.0 M values: 5.9 ms).
    """

    INF = 10e19

    def __init__(self, obj, obj_grad, equations_of_motion, state_symbols,
                 num_collocation_nodes, node_time_interval,
                 known_parameter_map={}, known_trajectory_map={},
                 instance_constraints=None, time_symbol=None, tmp_dir=None,
                 integration_method='backward euler', parallel=False,
                 bounds=None, show_compile_output=False, backend='hip',
                 eom_bounds=None, device=0, prune_zeros=False,
                 jacobian_layout='coo', deterministic=False,
                 verify_builds=None, specialize_parameters=None,
                 obj_hessian=None):
        if obj_hessian is not None:
            obj_hessian = self._check_obj_hessian(obj_hessian)
        if not sm.Matrix(equations_of_motion).has(sm.Derivative):
            raise ValueError('No time derivatives are present. The equations '
                             'of motion must be ordinary differential '
                             'equations (ODEs) or differential algebraic '
                             'equations (DAEs).')
        self.collocator = self._make_collocator(
            equations_of_motion, state_symbols, num_collocation_nodes,
            node_time_interval, known_parameter_map, known_trajectory_map,
            instance_constraints, time_symbol, tmp_dir, integration_method,
            parallel, show_compile_output=show_compile_output,
            backend=backend, device=device, prune_zeros=prune_zeros,
            jacobian_layout=jacobian_layout, deterministic=deterministic,
            verify_builds=verify_builds,
            specialize_parameters=specialize_parameters)
        self._bounds = bounds
        if eom_bounds is not None:
            bad = [k for k in eom_bounds
                   if k not in range(self.collocator.num_eom)]
            if bad:
                raise ValueError(f'Keys {bad} in eom_bounds do not '
                                 'correspond to equations of motion.')
        self._eom_bounds = eom_bounds

        def nargs(f):
            return f.__code__.co_argcount - len(f.__defaults__ or ())
        self._obj_num_args, self._obj_grad_num_args = nargs(obj), \
            nargs(obj_grad)
        if self._obj_num_args not in (1, 2):
            raise ValueError('The objective function can only have one or '
                             'two arguments.')
        if self._obj_grad_num_args not in (1, 2):
            raise ValueError('The gradient function can only have one or two'
                             ' arguments.')
        self.obj, self.obj_grad = obj, obj_grad
        (self.con, self.con_jac, self.con_jac_rows,
         self.con_jac_cols) = self._make_callbacks()
        self.num_free = self.collocator.num_free
        self.num_constraints = self.collocator.num_constraints
        self._generate_bound_arrays()
        self._generate_constraint_bound_arrays()
        self.obj_value = []
        self._nlp = None
        if obj_hessian is not None:
            self._install_hessian(obj_hessian)

    @staticmethod
    def _check_obj_hessian(obj_hessian):
        """``(rows, cols, values)`` of the objective's Hessian: int64
        indices of its lower triangle (``row >= col``), ``values`` a callable
        of ``free`` or of ``(problem, free)``."""
        try:
            rows, cols, values = obj_hessian
        except (TypeError, ValueError):
            raise ValueError('obj_hessian must be (rows, cols, values).')
        rows = np.asarray(rows, dtype=np.int64).ravel()
        cols = np.asarray(cols, dtype=np.int64).ravel()
        if rows.shape != cols.shape:
            raise ValueError('obj_hessian rows and cols differ in length.')
        if np.any(rows < cols):
            raise ValueError('obj_hessian must hold the lower triangle only '
                             '(row >= col).')
        if not callable(values):
            raise ValueError('obj_hessian values must be a callable of free '
                             'or of (problem, free).')
        return rows, cols, values

    def _objective_hessian_of(self, obj_hessian):
        """``(rows, cols, values, nargs, device_backed)`` of a checked
        ``obj_hessian`` for this problem: the indices within ``num_free``,
        ``nargs`` the number of arguments ``values`` takes (1 or 2), and
        whether ``values`` is device-backed
        (``create_objective_hessian_function``): it then applies
        ``obj_factor`` itself and can fill a device buffer in place."""
        rows, cols, values = obj_hessian
        if np.any((rows < 0) | (rows >= self.num_free)):
            raise ValueError('obj_hessian indices out of range.')
        nargs = values.__code__.co_argcount - len(values.__defaults__ or ()) \
            if hasattr(values, '__code__') else 1
        return rows, cols, values, nargs, isinstance(
            getattr(values, 'handle', None), hb.HipObjectiveHessian)

    def _install_hessian(self, obj_hessian):
        """Gives this instance the two callbacks cyipopt looks for --
        ``hessianstructure()`` and ``hessian(free, lagrange, obj_factor)``:
        the constraint triplets (``generate_hessian_function``, lower
        triangle, summed duplicates), then the objective's.  Only an instance
        built with ``obj_hessian`` has them; without them IPOPT keeps its
        limited-memory quasi-Newton default."""
        rows, cols, values, nargs, device_backed = \
            self._objective_hessian_of(obj_hessian)
        col = self.collocator
        con_hess = col.generate_hessian_function()
        crows, ccols = col.hessian_indices()
        structure = (np.concatenate((crows, rows)),
                     np.concatenate((ccols, cols)))
        num_con = len(crows)

        def hessianstructure():
            return structure

        def hessian(free, lagrange, obj_factor):
            if on_device(free):
                if not device_backed:
                    raise TypeError(
                        'Problem.hessian with torch CUDA tensors needs an '
                        'obj_hessian whose values have a device handle '
                        '(values.handle: opty_amd.create_objective_hessian_'
                        'function); a hand-written values callable works on '
                        'host arrays only.')
                import torch
                chess = con_hess(free, lagrange)
                out = torch.empty(num_con + len(rows), dtype=torch.float64,
                                  device=chess.device)
                out[:num_con] = chess
                values(free, obj_factor, out[num_con:])
                return out
            out = np.empty(num_con + len(rows))
            out[:num_con] = con_hess(free, lagrange)
            if device_backed:
                values(free, obj_factor, out[num_con:])
                return out
            v = values(self, free) if nargs == 2 else values(free)
            out[num_con:] = obj_factor*np.asarray(v, dtype=float)
            return out
        self.hessianstructure = hessianstructure
        self.hessian = hessian

        def objective_handle(method):
            """The device handle of ``values``, of this problem's sizes."""
            if not device_backed:
                raise TypeError(
                    'Problem.%s needs an obj_hessian whose '
                    'values have a device handle (values.handle: opty_amd.'
                    'create_objective_hessian_function); a hand-written '
                    'values callable has no index pattern to fuse.' % method)
            objective = values.handle
            prog = col._build_hessian_program()
            want = dict(N=col.num_collocation_nodes, n=prog.n, q=prog.q,
                        r=prog.r)
            have = {k: objective.desc[k] for k in want}
            if have != want or prog.s:
                raise ValueError(
                    'the objective Hessian was built for %s, the problem '
                    'has %s' % (have, dict(want, s=prog.s)))
            return objective

        def hessian_operator(free, lagrange, obj_factor=1.0):
            """The Hessian of the Lagrangian at ``(free, lagrange,
            obj_factor)`` -- constraint triplets, then the objective's -- as
            a ``scipy.sparse.linalg.LinearOperator`` of shape ``(num_free,
            num_free)`` (:meth:`ConstraintCollocator.hessian_operator`): the
            triplets are evaluated once into a device buffer that the
            operator owns (``.values``), every product runs on the GPU.
            Needs a device-backed ``obj_hessian``
            (``opty_amd.create_objective_hessian_function``)."""
            objective = objective_handle('hessian_operator')
            handle = col._ensure_hessmv(objective)
            if not on_device(free):
                free = col._host_free(free)
            return col._hessian_operator(
                handle, hessian(free, lagrange, obj_factor))
        self.hessian_operator = hessian_operator

        def hessian_csr_structure():
            """``(indptr, indices)`` (int64) of the Hessian of the
            Lagrangian -- the ``[constraint | objective]`` triplets of
            ``hessianstructure()`` -- as the CSR lower triangle over
            ``num_free`` rows, every pair once, rows and columns ascending
            (:meth:`ConstraintCollocator.hessian_csr_structure`).  Needs a
            device-backed ``obj_hessian``."""
            handle = col._ensure_hesscsr(
                objective_handle('hessian_csr_structure'))
            return col._csr_structure_of(handle, col.num_free,
                                         handle.nnz_unique)

        csr = {}

        def hessian_csr(free, lagrange, obj_factor=1.0):
            """``data`` of ``hessian_csr_structure()`` at ``(free, lagrange,
            obj_factor)``: the triplets of ``hessian(...)`` compressed on the
            GPU, the triplets of a pair summed in a fixed order
            (:meth:`ConstraintCollocator.generate_hessian_csr_function`).
            Host arrays in: a persistent page-locked array out; torch CUDA
            tensors in: a new CUDA tensor out."""
            handle = col._ensure_hesscsr(objective_handle('hessian_csr'))
            if csr.get('handle') is not handle:
                csr.update(handle=handle,
                           compress=col._hessian_csr_compress(handle))
            if not on_device(free):
                free = col._host_free(free)
            return csr['compress'](hessian(free, lagrange, obj_factor))
        self.hessian_csr_structure = hessian_csr_structure
        self.hessian_csr = hessian_csr

        def kkt_csr_structure():
            """``(indptr, indices)`` (int64) of the lower triangle of the
            augmented system ``[[W + diag(sigma) + delta_w I, J^T], [J,
            -delta_c I]]`` over ``num_free + num_constraints`` rows, ``W``
            the Hessian of the Lagrangian over the ``[constraint |
            objective]`` triplets, every diagonal stored and last in its row
            (:meth:`ConstraintCollocator.kkt_csr_structure`).  Needs
            ``jacobian_layout='csr'`` and a device-backed ``obj_hessian``."""
            col._require_csr_layout('Problem.kkt_csr_structure')
            handle = col._ensure_kktcsr(objective_handle('kkt_csr_structure'))
            return col._csr_structure_of(
                handle, col.num_free + col.num_constraints, handle.nnz_kkt)

        kkt = {}

        def hessian_into(free, lagrange, out, obj_factor):
            # the constraint section on the collocator's stream, the
            # objective's on torch's: the assembly waits for both
            col._ensure_hessian().evaluate(free, lagrange, out[:num_con],
                                           hb.DEVICE)
            values(free, obj_factor, out[num_con:])

        def kkt_csr(free, lagrange, obj_factor=1.0, sigma=None, delta_w=0.0,
                    delta_c=0.0):
            """``data`` of ``kkt_csr_structure()`` at ``(free, lagrange,
            obj_factor)``, assembled on the GPU from the triplets of
            ``hessian(...)`` and the Jacobian's values, none of which leaves
            the device
            (:meth:`ConstraintCollocator.generate_kkt_csr_function`): a
            diagonal of the ``W`` block is ``(h + sigma_r) + delta_w``, one
            of the constraint block ``0.0 - delta_c``.  Host arrays in: a
            persistent page-locked array out; torch CUDA tensors in: a new
            CUDA tensor out."""
            col._require_csr_layout('Problem.kkt_csr')
            handle = col._ensure_kktcsr(objective_handle('kkt_csr'))
            if kkt.get('handle') is not handle:
                kkt.update(handle=handle, function=col._kkt_csr_function(
                    handle, hessian_into))
            function = kkt['function']
            if on_device(free):
                return function(free, lagrange, obj_factor, sigma=sigma,
                                delta_w=delta_w, delta_c=delta_c)
            import torch
            device = torch.device('cuda', col._device)
            free, lagrange, sigma = (
                x if x is None else torch.from_numpy(x).to(device)
                for x in host_vectors((
                    (free, 'free', col.num_free),
                    (lagrange, 'lagrange', col.num_constraints),
                    (sigma, 'sigma', col.num_free))))
            out = function(free, lagrange, obj_factor, sigma=sigma,
                           delta_w=delta_w, delta_c=delta_c)
            result = function.assemble.result
            result[:] = out.cpu().numpy()
            return result
        self.kkt_csr_structure = kkt_csr_structure
        self.kkt_csr = kkt_csr

    bounds = property(lambda self: self._bounds)
    eom_bounds = property(lambda self: self._eom_bounds)

    # -- what a subclass replaces to evaluate elsewhere (ShardedProblem) ------
    def _make_collocator(self, *args, **kwargs):
        return ConstraintCollocator(*args, **kwargs)

    def _make_callbacks(self):
        """``(constraints, jacobian, rows, cols)``."""
        rows, cols = self.collocator.jacobian_indices()
        # (cyipopt copies what a callback returns before it calls the next)
        return (self.collocator.generate_constraint_function(recycle=True),
                self.collocator.generate_jacobian_function(), rows, cols)

    # -- bounds (opty/direct_collocation.py:370-440) -----------------------
    def _generate_constraint_bound_arrays(self):
        lo = np.zeros(self.num_constraints)
        hi = np.zeros(self.num_constraints)
        if self.eom_bounds is not None:
            span = self.collocator.num_collocation_nodes - 1
            for j, (a, b) in self.eom_bounds.items():
                lo[j*span:(j + 1)*span] = a
                hi[j*span:(j + 1)*span] = b
        self._low_con_bounds, self._upp_con_bounds = lo, hi

    def _generate_bound_arrays(self):
        col = self.collocator
        N = col.num_collocation_nodes
        lb = -self.INF*np.ones(self.num_free)
        ub = self.INF*np.ones(self.num_free)
        tail = N*(col.num_states + col.num_unknown_input_trajectories)
        for var, (lo, hi) in (self.bounds or {}).items():
            if var in col.state_symbols:
                start = col.state_symbols.index(var)*N
                sl = slice(start, start + N)
            elif var in col.unknown_input_trajectories:
                start = (col.num_states +
                         col.unknown_input_trajectories.index(var))*N
                sl = slice(start, start + N)
            elif var in col.unknown_parameters:
                k = tail + col.unknown_parameters.index(var)
                sl = slice(k, k + 1)
            elif (col._variable_duration and
                  var == col.time_interval_symbol):
                sl = slice(self.num_free - 1, self.num_free)
            else:
                raise ValueError('Bound variable {} not present in free '
                                 'variables.'.format(var))
            lb[sl] = lo
            ub[sl] = hi
        self.lower_bound, self.upper_bound = lb, ub

    # -- IPOPT callbacks (opty/direct_collocation.py:442-567) ---------------
    def objective(self, free):
        return self.obj(*((self, free)[2 - self._obj_num_args:]))

    def gradient(self, free):
        return self.obj_grad(*((self, free)[2 - self._obj_grad_num_args:]))

    def constraints(self, free):
        return self.con(free)

    def jacobianstructure(self):
        return (self.con_jac_rows, self.con_jac_cols)

    def jacobian(self, free):
        return self.con_jac(free)

    def jacobian_operator(self, free):
        """The constraint Jacobian at ``free`` as a matrix-free
        ``scipy.sparse.linalg.LinearOperator``
        (:meth:`ConstraintCollocator.jacobian_operator`)."""
        return self.collocator.jacobian_operator(free)

    def normal_operator(self, free, d=None, delta_c=0.0):
        """The inverse of the constraint normal matrix at ``free`` as a
        ``scipy.sparse.linalg.LinearOperator``
        (:meth:`ConstraintCollocator.normal_operator`)."""
        return self.collocator.normal_operator(free, d, delta_c)

    def intermediate(self, *args):
        self.obj_value.append(args[2])

    # -- helpers ------------------------------------------------------------
    def _extraction_map(self):
        """``{variable: slice of the free vector}`` for every unknown
        (``opty/direct_collocation.py:972-1002``)."""
        col = self.collocator
        N, n = col.num_collocation_nodes, col.num_states
        q = col.num_unknown_input_trajectories
        d = {}
        for k, var in enumerate(col.state_symbols):
            d[var] = range(k*N, (k + 1)*N)
        for k, var in enumerate(col.unknown_input_trajectories):
            d[var] = range((n + k)*N, (n + k + 1)*N)
        for k, var in enumerate(col.unknown_parameters):
            d[var] = range((n + q)*N + k, (n + q)*N + k + 1)
        if col._variable_duration:
            d[col.time_interval_symbol] = range(self.num_free - 1,
                                                self.num_free)
        return d

    def _indices_of(self, variables):
        d = self._extraction_map()
        idxs = []
        for var in variables:
            try:
                idxs += list(d[var])
            except KeyError:
                raise ValueError(f'{var} not an unknown in this problem.')
        return idxs

    def fill_free(self, free, values, *variables):
        """Writes ``values`` into the entries of ``free`` that belong to
        ``variables`` (``opty/direct_collocation.py:1004-1030``)."""
        free[self._indices_of(variables)] = values

    def extract_values(self, free, *variables):
        """The entries of ``free`` that belong to ``variables``
        (``opty/direct_collocation.py:1032-1054``)."""
        return free[self._indices_of(variables)]

    def check_bounds_conflict(self, free):
        """Raises ``ValueError`` if a lower bound exceeds its upper bound or
        the guess ``free`` violates a bound
        (``opty/direct_collocation.py:317-368``)."""
        reversed_bounds = []
        if self.eom_bounds is not None:
            reversed_bounds += [k for k, (lo, hi) in self.eom_bounds.items()
                                if lo > hi]
        if self.bounds is not None:
            violating = []
            for sym, (lo, hi) in self.bounds.items():
                if np.any(lo > hi):
                    reversed_bounds.append(sym)
                vals = self.extract_values(free, sym)
                if np.any(vals < lo) or np.any(vals > hi):
                    violating.append(sym)
            if violating:
                raise ValueError(f'The initial guesses for {violating} are '
                                 'in conflict with their bounds.')
        if reversed_bounds:
            raise ValueError(f'The lower bound(s) for {reversed_bounds} is '
                             '(are) greater than the upper bound(s).')

    def parse_free(self, free):
        col = self.collocator
        return parse_free(free, col.num_states,
                          col.num_unknown_input_trajectories,
                          col.num_collocation_nodes,
                          variable_duration=col._variable_duration)

    def time_vector(self, solution=None, start_time=0.0):
        col = self.collocator
        N = col.num_collocation_nodes
        if col._variable_duration:
            if solution is None:
                raise ValueError('Solution vector must be provided for '
                                 'variable duration.')
            h = float(solution[-1])
            if h <= 0.0:
                raise ValueError('Time interval must be strictly greater '
                                 'than zero.')
            if start_time >= h*(N - 1):
                raise ValueError('Start time must be less than the final '
                                 'time.')
        else:
            h = col.node_time_interval
        return np.linspace(start_time, start_time + (N - 1)*h, num=N)

    def _ipopt(self):
        if self._nlp is None:
            try:
                import cyipopt
            except ImportError as err:
                raise ImportError('Problem.solve needs cyipopt (IPOPT), which '
                                  'is not installed.') from err
            self._nlp = cyipopt.Problem(
                n=self.num_free, m=self.num_constraints, problem_obj=self,
                lb=self.lower_bound, ub=self.upper_bound,
                cl=self._low_con_bounds, cu=self._upp_con_bounds)
        return self._nlp

    def add_option(self, *args, **kwargs):
        return self._ipopt().add_option(*args, **kwargs)

    def solve(self, free, lagrange=[], zl=[], zu=[], respect_bounds=False):
        if respect_bounds:
            self.check_bounds_conflict(free)
        return self._ipopt().solve(free, lagrange=lagrange, zl=zl, zu=zu)


class ShardedProblem(Problem):
    """``Problem`` whose ``constraints`` / ``jacobian`` callbacks are evaluated
    by all GPUs of a node (BASELINE config 4; one process per GPU,
    ``torch.distributed`` initialised by the caller).

    Every rank constructs it with the same arguments.  The rank that runs the
    solver (``root``) uses it like a ``Problem`` (``solve``, or the callbacks
    directly) and calls :meth:`shutdown` when done; every other rank calls
    :meth:`serve`, which returns after the shutdown.  The collocation nodes are
    sharded (:class:`opty_amd.sharded.ShardedCollocator`), each rank copies its
    shard of every result over its own PCIe link into host vectors shared by
    all processes (:class:`opty_amd.sharded.ShardedCallbacks`).  Instance
    constraints (their tails are evaluated once per call from the global
    ``free``), known trajectories given as functions of ``free`` and changes of
    the ROOT's known maps between solves are all supported; the CSR layout is
    not sharded.

    :meth:`jacobian_operator` gives the matrix-free products ``J v`` / ``J^T
    w`` of the sharded problem; block products and ``ufuncify_matrix`` are
    not sharded.

    ``obj_hessian=(rows, cols, values)`` (``Problem``'s argument, with its
    checks) gives the root the two callbacks of the exact Hessian
    (DESIGN.md section 9.2): ``hessianstructure()`` is the ``[constraint |
    objective]`` structure of ``Problem``, and in ``hessian(free, lagrange,
    obj_factor)`` every rank evaluates the constraint triplets of its own
    nodes (:meth:`opty_amd.sharded.ShardedCallbacks.hessian`: every value has
    the bits of the single-GPU ``Problem.hessian``) while the root alone
    evaluates the objective's -- on its GPU when ``values.handle`` is a
    ``HipObjectiveHessian`` -- behind them in the same shared host vector,
    which is returned and overwritten by the next call.  Host arrays only.
    ``values`` is only ever called on the root.  What
    ``generate_hessian_function`` refuses (implicit known trajectories,
    known trajectories given as functions of ``free``) is refused by the
    constructor on every rank, before any collective; so is ``obj_hessian``
    in a process without an initialised ``torch.distributed`` group
    (``NotImplementedError``: there are no ranks to serve it).

    :meth:`resident_hessian_operator` gives ``H v`` from shards that stay in
    device memory: one load, then one round of
    ``num_free`` doubles each way per product; :meth:`hessian_operator`
    itself keeps refusing.  Not sharded: the objective's Hessian (the root
    alone evaluates and multiplies it), block products, ``hessian_csr`` /
    ``kkt_csr``, ``normal_operator``; the torch-free host (``shard_host.py``) and the C client
    do not serve the Hessian.

    Extra keywords: ``group`` (process group), ``root`` (solver rank),
    ``torch_device`` (default ``cuda:<device>``), ``sharded_kwargs`` (further
    keywords of :class:`opty_amd.sharded.ShardedCollocator`: the evaluators
    the CPU tests inject).
    """

    def __init__(self, *args, group=None, root=0, torch_device=None,
                 sharded_kwargs=None, **kwargs):
        self._group, self._root, self._torch_device = group, root, \
            torch_device
        self._sharded_kwargs = dict(sharded_kwargs or {})
        self._with_hessian = kwargs.get('obj_hessian') is not None
        if self._with_hessian:
            # the first of the refusals that come before any collective: the
            # sharded Hessian is what the ranks of a process group evaluate
            # on the root's command, and without a group there are none
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized()):
                raise NotImplementedError(
                    'the Hessian of a ShardedProblem is evaluated by the '
                    'ranks of a torch.distributed process group, and none '
                    'is initialised: there is nothing to shard over.  Use '
                    'Problem(obj_hessian=...) in a single process.')
        super().__init__(*args, **kwargs)

    def hessian_operator(self, free, lagrange, obj_factor=1.0):
        raise NotImplementedError('the Hessian is not sharded: '
                                  'ShardedProblem has no hessian_operator.')

    def hessian_csr_structure(self):
        raise NotImplementedError(
            'the Hessian is not sharded: ShardedProblem has no '
            'hessian_csr_structure.')

    def hessian_csr(self, free, lagrange, obj_factor=1.0):
        raise NotImplementedError('the Hessian is not sharded: '
                                  'ShardedProblem has no hessian_csr.')

    def kkt_csr_structure(self):
        raise NotImplementedError(
            'the Hessian is not sharded: ShardedProblem has no '
            'kkt_csr_structure.')

    def kkt_csr(self, free, lagrange, obj_factor=1.0, sigma=None,
                delta_w=0.0, delta_c=0.0):
        raise NotImplementedError('the Hessian is not sharded: '
                                  'ShardedProblem has no kkt_csr.')

    def normal_operator(self, free, d=None, delta_c=0.0):
        raise NotImplementedError(
            'the normal-matrix solver is not sharded: ShardedProblem has '
            'no normal_operator.')

    def _install_hessian(self, obj_hessian):
        """``hessianstructure()`` and ``hessian(free, lagrange,
        obj_factor)`` of :meth:`Problem._install_hessian`, the constraint
        section served by all ranks.  Every rank gets here (the size of the
        shared vector is agreed without communication); only the root holds
        the structure and ever calls ``values``."""
        rows, cols, values, nargs, device_backed = \
            self._objective_hessian_of(obj_hessian)
        cb, col = self.callbacks, self.collocator
        cb.hessian_extra = len(rows)
        # (what resident_hessian_operator needs of the objective)
        self._objective_parts = (rows, values, device_backed)
        if not cb.is_root:
            return
        num_con = self.sharded.hessian_nnz
        # (the closed form on the host: the device's index kernel is held to
        # it by the tests, and the root need not build its handle for it)
        crows, ccols = col.hessian_indices_closed_form()
        assert len(crows) == num_con
        structure = (np.concatenate((crows, rows)),
                     np.concatenate((ccols, cols)))
        obj_dev = []

        def hessianstructure():
            return structure

        def hessian(free, lagrange, obj_factor):
            if on_device(free) or on_device(lagrange):
                raise TypeError(
                    'ShardedProblem.hessian takes host arrays only: the '
                    'result is assembled in a host vector shared by the '
                    'ranks, not in one GPU\'s memory; pass NumPy arrays '
                    '(free.cpu().numpy()).')
            free = col._host_free(free)
            out = cb.hessian(free, lagrange)
            if not len(rows):
                return out
            if device_backed:
                # the root's own GPU, into the (page-locked) shared vector
                # behind the constraint section
                import torch
                if not obj_dev:
                    obj_dev.append(torch.empty(
                        len(rows), dtype=torch.float64,
                        device=self.sharded.device))
                values(cb.free_dev, obj_factor, obj_dev[0])
                cb.hess_host.torch_view(num_con, num_con + len(rows)).copy_(
                    obj_dev[0])
                return out
            v = values(self, free) if nargs == 2 else values(free)
            out[num_con:] = obj_factor*np.asarray(v, dtype=float)
            return out
        self.hessianstructure = hessianstructure
        self.hessian = hessian

    def _make_collocator(self, eom, states, num_nodes, interval, par_map,
                         traj_map, instance_constraints, time_symbol, tmp_dir,
                         integration_method, parallel, **kwargs):
        from .sharded import ShardedCollocator
        device = self._torch_device
        if device is None:
            device = 'cuda:%d' % kwargs.get('device', 0)
        kwargs.pop('device', None)
        kwargs.update(self._sharded_kwargs)
        self.sharded = ShardedCollocator(
            eom, states, num_nodes, interval, par_map, traj_map,
            instance_constraints, group=self._group, device=device,
            time_symbol=time_symbol, tmp_dir=tmp_dir,
            integration_method=integration_method, parallel=parallel,
            **kwargs)
        if self._with_hessian:
            # what generate_hessian_function refuses (implicit known
            # trajectories, known trajectories as functions of free) is
            # refused here, on every rank, before the first collective: a
            # refusal inside one would leave the other ranks waiting
            self.sharded.collocator._build_hessian_program()
        return self.sharded.collocator

    def _make_callbacks(self):
        from .sharded import ShardedCallbacks
        self.callbacks = ShardedCallbacks(self.sharded, root=self._root)
        rows = cols = None
        if self.callbacks.is_root:       # the structure goes to the solver
            rows, cols = self.collocator.jacobian_indices()
        return (self.callbacks.constraints, self.callbacks.jacobian, rows,
                cols)

    def _resident_objective(self):
        """Root: ``(values, product handle)`` of the objective section of
        :meth:`resident_hessian_operator`, or None for an ``obj_hessian``
        without entries.  Refuses, before any collective, what
        ``Problem.hessian_operator`` refuses."""
        parts = getattr(self, '_objective_parts', None)
        if parts is None:
            raise NotImplementedError(
                'ShardedProblem.resident_hessian_operator needs a problem '
                'built with obj_hessian=(rows, cols, values): the ranks '
                'agree on the Hessian at construction, before any '
                'collective.')
        rows, values, device_backed = parts
        if not len(rows):
            return None
        if not device_backed:
            raise TypeError(
                'ShardedProblem.resident_hessian_operator needs an '
                'obj_hessian whose values have a device handle '
                '(values.handle: opty_amd.create_objective_hessian_'
                'function); a hand-written values callable has no index '
                'pattern to multiply with.')
        col = self.collocator
        objective = values.handle
        prog = col._build_hessian_program()
        want = dict(N=col.num_collocation_nodes, n=prog.n, q=prog.q,
                    r=prog.r)
        have = {k: objective.desc[k] for k in want}
        if have != want or prog.s:
            raise ValueError(
                'the objective Hessian was built for %s, the problem has %s'
                % (have, dict(want, s=prog.s)))
        if getattr(self, '_resident_objective_of', None) is not objective:
            # the objective section alone (PH = 0), over the root's problem
            # handle
            tail = (prog.n + prog.q)*col.num_collocation_nodes
            self._resident_objective_handle = hb.HipHessianProduct(
                col.hip, dict(obj_pattern=objective.pattern,
                              obj_base=objective.desc['base'],
                              tail_rows=tail + objective.tail_pairs[:, 0],
                              tail_cols=tail + objective.tail_pairs[:, 1]))
            self._resident_objective_of = objective
        return values, self._resident_objective_handle

    def resident_hessian_operator(self, free, lagrange, obj_factor=1.0):
        """Root: the Hessian of the Lagrangian at ``(free, lagrange,
        obj_factor)`` as a symmetric ``scipy.sparse.linalg.LinearOperator``
        of shape ``(num_free, num_free)`` whose values never leave the GPUs
        (the serving ranks answer from
        :meth:`serve`).  The call loads the values ONCE: every rank
        evaluates the constraint triplets of its own nodes, and of one halo
        node, into its device memory
        (:meth:`opty_amd.sharded.ShardedCallbacks.hessian_load`); every
        ``matvec`` is then one round in which each rank multiplies its
        window (``opty_hip_hessmv_apply_shard``) and ``num_free`` doubles
        travel each way.  The trajectory entries of the constraint part have
        the bits of the single-GPU ``hessian_operator``'s, its
        node-invariant tail is the sum of the ranks' shares in rank order.
        ``matmat`` loops over the columns: block products are not sharded.

        The objective section is the root's alone: it evaluates the
        objective's values into a device buffer of its own and multiplies
        them with an objective-only product handle; the result is
        ``y_con + y_obj``, one rounding per element.  This needs a
        device-backed ``obj_hessian``
        (``opty_amd.create_objective_hessian_function``) -- anything else is
        refused as ``Problem.hessian_operator`` refuses it, before any
        collective --; an ``obj_hessian`` without entries skips the section.

        Host arrays only (``TypeError`` for a CUDA tensor).  The name
        differs from :meth:`hessian_operator` because the contract does: the
        values live on all ranks and ONE set is resident at a time.  A later
        ``resident_hessian_operator`` (or ``callbacks.hessian_load``)
        replaces it; a product through an older operator then raises
        ``RuntimeError``."""
        from scipy.sparse.linalg import LinearOperator
        if on_device(free) or on_device(lagrange):
            raise TypeError(
                'ShardedProblem.resident_hessian_operator takes host arrays '
                'only: the vectors travel through host memory shared by the '
                'ranks; pass NumPy arrays (free.cpu().numpy()).')
        objective = self._resident_objective()
        cb, col, sh = self.callbacks, self.collocator, self.sharded
        free = col._host_free(free)
        nfree = sh._num_free()
        generation = cb.hessian_load(free, lagrange)
        obj_values = None
        if objective is not None:
            import torch
            values, handle = objective
            obj_values = torch.empty(handle.nnz, dtype=torch.float64,
                                     device=sh.device)
            # (cb.free_dev: where the load left free on the root's GPU)
            values(cb.free_dev, obj_factor, obj_values)
            y_obj = torch.empty(nfree, dtype=torch.float64, device=sh.device)

        def product(x):
            y = cb.hmv(np.asarray(x, dtype=np.float64).reshape(-1),
                       generation)
            if obj_values is None:
                return y
            # (cb._hv_dev: where the round left v on the root's GPU)
            import torch
            sh._use_stream()
            handle.apply(obj_values, cb._hv_dev, y_obj, hb.DEVICE)
            torch.cuda.synchronize(sh.device)
            return y + y_obj.cpu().numpy()

        class ResidentHessianOperator(LinearOperator):
            def __init__(op):
                super().__init__(np.dtype(np.float64), (nfree, nfree))

            def _matvec(op, x):
                return product(x)

            _rmatvec = _matvec

            def _matmat(op, X):
                X = np.asarray(X, dtype=np.float64)
                out = np.empty((nfree, X.shape[1]))
                for c in range(X.shape[1]):
                    out[:, c] = product(X[:, c])
                return out

            _rmatmat = _matmat

        op = ResidentHessianOperator()
        op.generation = generation
        return op

    def jacobian_operator(self, free):
        """Root: the constraint Jacobian at ``free`` as the
        ``scipy.sparse.linalg.LinearOperator`` of
        :meth:`Problem.jacobian_operator` -- shape ``(num_constraints,
        num_free)``, float64 -- whose ``matvec`` / ``rmatvec`` are evaluated
        by all ranks, each on its window of the constraint nodes
        (:meth:`opty_amd.sharded.ShardedCallbacks.jvp` / ``vjp``; the serving
        ranks answer from :meth:`serve`).  Every entry but the node-invariant
        tail of ``J^T w`` has the bits of the single-GPU operator's; the tail
        is the sum of the ranks' shares in rank order.  ``matmat`` /
        ``rmatmat`` loop over the columns: block products, like the Hessian
        and ``ufuncify_matrix``, are not sharded."""
        from scipy.sparse.linalg import LinearOperator
        cb = self.callbacks
        free = np.array(free, dtype=np.float64).reshape(-1)
        shape = (self.sharded.num_constraints, self.sharded._num_free())

        def columns(f, X, rows):
            X = np.asarray(X, dtype=np.float64)
            out = np.empty((rows, X.shape[1]))
            for c in range(X.shape[1]):
                out[:, c] = f(free, X[:, c])
            return out

        class ShardedJacobianOperator(LinearOperator):
            def __init__(op):
                super().__init__(np.dtype(np.float64), shape)

            def _matvec(op, x):
                return cb.jvp(free, np.asarray(x).reshape(-1))

            def _rmatvec(op, x):
                return cb.vjp(free, np.asarray(x).reshape(-1))

            def _matmat(op, X):
                return columns(cb.jvp, X, shape[0])

            def _rmatmat(op, X):
                return columns(cb.vjp, X, shape[1])

        return ShardedJacobianOperator()

    def serve(self):
        """Non-root ranks: evaluate on the root's command until shutdown."""
        self.callbacks.serve()

    def shutdown(self):
        """Root: release the serving ranks."""
        self.callbacks.shutdown()
