// solve_many and fcg_periodic_many of the C++ mirror on a periodic 2D solver (include/cedar/2d/solver.h: the keys
// solver.max-rhs and solver.periodic-batch; include/cedar/multilevel.h), driven by tests/test_cxx_periodic_many2d.py: the
// periodic five-point Poisson operator of examples/ser-periodic-2d.cc with three rational or integer right-hand sides (no
// libm call, so that the Python side forms the same bits), the ghost layers of b filled with garbage.  Histories,
// iteration counts and three rows of every x (the first, a middle and the last interior row) are printed as one JSON
// line; without solver.periodic-batch the solver holds one right-hand side and both calls are refused (empty histories).
//   periodic_many2d <configuration file>
#include <array>
#include <cstdio>
#include <string>
#include <cedar/2d/solver.h>

using namespace cedar;

static cdr2::stencil_op<cdr2::five_pt> create_op2(len_t nx, len_t ny, std::array<bool, 3> periodic)
{
	using namespace cedar::cdr2;
	stencil_op<five_pt> so(nx, ny);
	so.set(0);
	const len_t mx = nx - (periodic[0] ? 1 : 0), my = ny - (periodic[1] ? 1 : 0);
	const real_t hx = 1.0 / (mx + 1), hy = 1.0 / (my + 1), xh = hy / hx, yh = hx / hy;
	const len_t l = so.shape(0), m = so.shape(1);
	const len_t ibeg = periodic[0] ? 1 : 2, jbeg = periodic[1] ? 1 : 2;
	for (len_t j = jbeg; j <= m; j++) for (len_t i = 1; i <= l; i++) so(i, j, five_pt::s) = 1.0 * yh;
	for (len_t j = 1; j <= m; j++) for (len_t i = ibeg; i <= l; i++) so(i, j, five_pt::w) = 1.0 * xh;
	for (auto j : so.range(1)) for (auto i : so.range(0)) so(i, j, five_pt::c) = 2 * xh + 2 * yh;
	const five_pt dirs[3] = { five_pt::c, five_pt::w, five_pt::s };
	if (periodic[0])
		for (auto j : so.range(1))
			for (auto d : dirs) {
				so(ibeg - 1, j, d) = so(l, j, d);
				so(l + 1, j, d) = so(ibeg, j, d);
			}
	if (periodic[1])
		for (auto i : so.range(0))
			for (auto d : dirs) {
				so(i, jbeg - 1, d) = so(i, m, d);
				so(i, m + 1, d) = so(i, jbeg, d);
			}
	return so;
}

// histories, iterations and the rows `rows` (offsets of their first element) of every x after one batched call
template <class S> static void report(const char * key, const S & s, const std::vector<cdr2::grid_func> & x,
                                      const std::array<std::size_t, 3> & rows, std::size_t nrow)
{
	std::printf("\"%s\": {\"iters\": [", key);
	for (std::size_t m = 0; m < s.iterations.size(); m++) std::printf("%s%d", m ? ", " : "", s.iterations[m]);
	std::printf("], \"hist\": [");
	for (std::size_t m = 0; m < s.histories.size(); m++) {
		std::printf("%s[", m ? ", " : "");
		for (std::size_t i = 0; i < s.histories[m].size(); i++) std::printf("%s%.17g", i ? ", " : "", s.histories[m][i]);
		std::printf("]");
	}
	std::printf("], \"x\": [");
	for (std::size_t m = 0; m < x.size(); m++) {
		std::printf("%s[", m ? ", " : "");
		for (std::size_t r = 0; r < rows.size(); r++)
			for (std::size_t i = 0; i < nrow; i++) std::printf("%s%.17g", r + i ? ", " : "", x[m].data()[rows[r] + i]);
		std::printf("]");
	}
	std::printf("]}");
}

int main(int argc, char ** argv)
{
	if (argc < 2) return 2;
	auto conf = std::make_shared<config>(argv[1]);
	log::status.on = false;
	auto params = build_kernel_params(*conf);
	const auto per = params->periodic;
	auto n = conf->getvec<len_t>("grid.n");
	if (n.size() != 2) return 2;
	const len_t nx = n[0], ny = n[1];
	const int nrhs = 3;
	auto so = create_op2(nx, ny, per);
	std::vector<cdr2::grid_func> b, x, xf;
	for (int m = 0; m < nrhs; m++) {
		b.emplace_back(nx, ny);
		x.emplace_back(nx, ny);
		xf.emplace_back(nx, ny);
		b[m].set(-7.5); // garbage in the ghost layers of b: they must not matter
		x[m].set(0);
		xf[m].set(0);
		for (len_t j = 1; j <= ny; j++)
			for (len_t i = 1; i <= nx; i++)
				b[m](i, j) = m == 0 ? 1.0 / (1.0 + i + 2.0 * j) : m == 1 ? ((i * 7 + j * 13) % 17) - 8.0 : 0.125 * (((i * 5 + j * 3) % 7) - 3.0);
	}
	cdr2::solver<cdr2::five_pt> s(so, conf);
	const std::size_t II = nx + 2;
	// rows j = 1, ny / 2, ny
	const std::array<std::size_t, 3> rows = {II, II * (ny / 2), II * ny};
	std::printf("{");
	s.solve_many(b, x);
	report("solve_many", s, x, rows, II);
	std::printf(", ");
	s.fcg_periodic_many(b, xf);
	report("fcg_periodic_many", s, xf, rows, II);
	std::printf("}\n");
	return 0;
}
