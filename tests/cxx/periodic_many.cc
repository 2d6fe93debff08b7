// solve_many and fcg_periodic_many of the C++ mirror on a periodic 3D solver (include/cedar/3d/solver.h: the keys
// solver.max-rhs and solver.periodic-batch; include/cedar/multilevel.h), driven by tests/test_cxx_periodic_many.py: the
// periodic seven-point Poisson operator of examples/ser-periodic-3d.cc with three rational or integer right-hand sides (no
// libm call, so that the Python side forms the same bits), the ghost layers of b filled with garbage.  Histories,
// iteration counts and three rows of every x (the first, a middle and the last interior row) are printed as one JSON
// line; without solver.periodic-batch the solver holds one right-hand side and both calls are refused (empty histories).
//   periodic_many <configuration file>
#include <array>
#include <cstdio>
#include <string>
#include <cedar/3d/solver.h>

using namespace cedar;

static cdr3::stencil_op<cdr3::seven_pt> create_op3(len_t nx, len_t ny, len_t nz, std::array<bool, 3> per)
{
	using namespace cedar::cdr3;
	stencil_op<seven_pt> so(nx, ny, nz);
	so.set(0);
	const len_t mx = nx - (per[0] ? 1 : 0), my = ny - (per[1] ? 1 : 0), mz = nz - (per[2] ? 1 : 0);
	const real_t hx = 1.0 / (mx + 1), hy = 1.0 / (my + 1), hz = 1.0 / (mz + 1);
	const real_t xh = hy * hz / hx, yh = hx * hz / hy, zh = hx * hy / hz;
	const len_t l = so.shape(0), m = so.shape(1), n = so.shape(2);
	const len_t ibeg = per[0] ? 1 : 2, jbeg = per[1] ? 1 : 2, kbeg = per[2] ? 1 : 2;
	for (len_t k = 1; k <= n; k++) for (len_t j = jbeg; j <= m; j++) for (len_t i = 1; i <= l; i++) so(i, j, k, seven_pt::ps) = 1.0 * yh;
	for (len_t k = 1; k <= n; k++) for (len_t j = 1; j <= m; j++) for (len_t i = ibeg; i <= l; i++) so(i, j, k, seven_pt::pw) = 1.0 * xh;
	for (len_t k = kbeg; k <= n; k++) for (len_t j = 1; j <= m; j++) for (len_t i = 1; i <= l; i++) so(i, j, k, seven_pt::b) = 1.0 * zh;
	for (auto k : so.range(2)) for (auto j : so.range(1)) for (auto i : so.range(0)) so(i, j, k, seven_pt::p) = 2.0 * xh + 2.0 * yh + 2.0 * zh;
	const seven_pt dirs[4] = { seven_pt::p, seven_pt::pw, seven_pt::ps, seven_pt::b };
	if (per[0])
		for (auto k : so.grange(2)) for (auto j : so.grange(1)) for (auto d : dirs) {
			so(ibeg - 1, j, k, d) = so(l, j, k, d);
			so(l + 1, j, k, d) = so(ibeg, j, k, d);
		}
	if (per[1])
		for (auto k : so.grange(2)) for (auto i : so.grange(0)) for (auto d : dirs) {
			so(i, jbeg - 1, k, d) = so(i, m, k, d);
			so(i, m + 1, k, d) = so(i, jbeg, k, d);
		}
	if (per[2])
		for (auto j : so.grange(1)) for (auto i : so.grange(0)) for (auto d : dirs) {
			so(i, j, kbeg - 1, d) = so(i, j, n, d);
			so(i, j, n + 1, d) = so(i, j, kbeg, d);
		}
	return so;
}

// histories, iterations and the rows `rows` (offsets of their first element) of every x after one batched call
template <class S> static void report(const char * key, const S & s, const std::vector<cdr3::grid_func> & x,
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
	if (n.size() != 3) return 2;
	const len_t nx = n[0], ny = n[1], nz = n[2];
	const int nrhs = 3;
	auto so = create_op3(nx, ny, nz, per);
	std::vector<cdr3::grid_func> b, x, xf;
	for (int m = 0; m < nrhs; m++) {
		b.emplace_back(nx, ny, nz);
		x.emplace_back(nx, ny, nz);
		xf.emplace_back(nx, ny, nz);
		b[m].set(-7.5); // garbage in the ghost layers of b: they must not matter
		x[m].set(0);
		xf[m].set(0);
		for (len_t k = 1; k <= nz; k++)
			for (len_t j = 1; j <= ny; j++)
				for (len_t i = 1; i <= nx; i++)
					b[m](i, j, k) = m == 0 ? 1.0 / (1.0 + i + 2.0 * j + 3.0 * k)
					              : m == 1 ? ((i * 7 + j * 13 + k * 29) % 17) - 8.0 : 0.125 * (((i * 5 + j * 3 + k * 11) % 7) - 3.0);
	}
	cdr3::solver<cdr3::seven_pt> s(so, conf);
	const std::size_t II = nx + 2, JJ = ny + 2;
	// rows (j, k) = (1, 1), (ny / 2, nz / 2), (ny, nz)
	const std::array<std::size_t, 3> rows = {II * JJ + II, II * (JJ * (nz / 2) + ny / 2), II * (JJ * nz + ny)};
	std::printf("{");
	s.solve_many(b, x);
	report("solve_many", s, x, rows, II);
	std::printf(", ");
	s.fcg_periodic_many(b, xf);
	report("fcg_periodic_many", s, xf, rows, II);
	std::printf("}\n");
	return 0;
}
