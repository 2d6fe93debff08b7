// solver::fcg_semidefinite of the C++ mirror (include/cedar/multilevel.h), driven by tests/test_cxx_semidefinite.py: the
// fully periodic Poisson operator (five-point in 2D, seven-point in 3D; zero row sums, the periodic image in ALL ghost
// cells, corners and edges included) with the key solver.semidefinite: true, a right-hand side that is NOT compatible
// (its mean is removed by the call).  Printed as one JSON line: the history, the mean of x and of |x| over the interior, the
// residual |P b - A x| / |P b| formed here on the host with the wrapped x, and whether pcg() refused the solver.
//   semidefinite <configuration file>
#include <cmath>
#include <cstdio>
#include <cedar/2d/solver.h>
#include <cedar/3d/solver.h>

using namespace cedar;

static cdr2::stencil_op<cdr2::five_pt> create_op2(len_t nx, len_t ny)
{
	using namespace cedar::cdr2;
	stencil_op<five_pt> so(nx, ny);
	so.set(0);
	const real_t hx = 1.0 / nx, hy = 1.0 / ny, xh = hy / hx, yh = hx / hy;
	for (len_t j = 1; j <= ny; j++)
		for (len_t i = 1; i <= nx; i++) {
			so(i, j, five_pt::s) = yh;
			so(i, j, five_pt::w) = xh;
			so(i, j, five_pt::c) = 2 * xh + 2 * yh;
		}
	const five_pt dirs[3] = { five_pt::c, five_pt::w, five_pt::s };
	for (auto d : dirs) {
		for (len_t j = 1; j <= ny; j++) { so(0, j, d) = so(nx, j, d); so(nx + 1, j, d) = so(1, j, d); }
		for (len_t i = 0; i <= nx + 1; i++) { so(i, 0, d) = so(i, ny, d); so(i, ny + 1, d) = so(i, 1, d); } // corners too
	}
	return so;
}

static cdr3::stencil_op<cdr3::seven_pt> create_op3(len_t nx, len_t ny, len_t nz)
{
	using namespace cedar::cdr3;
	stencil_op<seven_pt> so(nx, ny, nz);
	so.set(0);
	const real_t hx = 1.0 / nx, hy = 1.0 / ny, hz = 1.0 / nz;
	const real_t xh = hy * hz / hx, yh = hx * hz / hy, zh = hx * hy / hz;
	for (len_t k = 1; k <= nz; k++)
		for (len_t j = 1; j <= ny; j++)
			for (len_t i = 1; i <= nx; i++) {
				so(i, j, k, seven_pt::ps) = yh;
				so(i, j, k, seven_pt::pw) = xh;
				so(i, j, k, seven_pt::b) = zh;
				so(i, j, k, seven_pt::p) = 2 * xh + 2 * yh + 2 * zh;
			}
	const seven_pt dirs[4] = { seven_pt::p, seven_pt::pw, seven_pt::ps, seven_pt::b };
	for (auto d : dirs) { // x, then y over all i, then z over all i and j: edges and corners are filled
		for (len_t k = 1; k <= nz; k++)
			for (len_t j = 1; j <= ny; j++) { so(0, j, k, d) = so(nx, j, k, d); so(nx + 1, j, k, d) = so(1, j, k, d); }
		for (len_t k = 1; k <= nz; k++)
			for (len_t i = 0; i <= nx + 1; i++) { so(i, 0, k, d) = so(i, ny, k, d); so(i, ny + 1, k, d) = so(i, 1, k, d); }
		for (len_t j = 0; j <= ny + 1; j++)
			for (len_t i = 0; i <= nx + 1; i++) { so(i, j, 0, d) = so(i, j, nz, d); so(i, j, nz + 1, d) = so(i, j, 1, d); }
	}
	return so;
}

template <class S, class G> static void solve(S & s, const G & b, G & x)
{
	G xp(x);
	s.pcg(b, xp);
	std::printf("{\"pcg_len\": %zu, ", s.history.size());
	s.fcg_semidefinite(b, x);
	std::printf("\"hist\": [");
	for (std::size_t i = 0; i < s.history.size(); i++) std::printf("%s%.17g", i ? ", " : "", s.history[i]);
	std::printf("]");
}

int main(int argc, char ** argv)
{
	if (argc < 2) return 2;
	auto conf = std::make_shared<config>(argv[1]);
	log::status.on = false;
	auto n = conf->getvec<len_t>("grid.n");
	long double sx = 0, sa = 0, sb = 0, rr = 0, bb = 0;
	if (n.size() == 2) {
		const len_t nx = n[0], ny = n[1];
		auto so = create_op2(nx, ny);
		cdr2::grid_func b(nx, ny), x(nx, ny);
		b.set(-7.5); // garbage in the ghost layers of b: they must not matter
		x.set(0);
		for (len_t j = 1; j <= ny; j++)
			for (len_t i = 1; i <= nx; i++) { b(i, j) = 3.0 + 1.0 / (1.0 + i + 2.0 * j); sb += b(i, j); }
		cdr2::solver<cdr2::five_pt> s(so, conf);
		solve(s, b, x);
		const real_t mb = (real_t)(sb / ((long double)nx * ny));
		for (len_t j = 1; j <= ny; j++)
			for (len_t i = 1; i <= nx; i++) {
				using namespace cedar::cdr2;
				const real_t ax = so(i, j, five_pt::c) * x(i, j) - so(i, j, five_pt::w) * x(i - 1, j) - so(i + 1, j, five_pt::w) * x(i + 1, j)
				                  - so(i, j, five_pt::s) * x(i, j - 1) - so(i, j + 1, five_pt::s) * x(i, j + 1);
				const real_t r = (b(i, j) - mb) - ax;
				rr += (long double)r * r; bb += (long double)(b(i, j) - mb) * (b(i, j) - mb); sx += x(i, j); sa += std::fabs(x(i, j));
			}
		sx /= (long double)nx * ny; sa /= (long double)nx * ny;
	} else {
		const len_t nx = n[0], ny = n[1], nz = n[2];
		auto so = create_op3(nx, ny, nz);
		cdr3::grid_func b(nx, ny, nz), x(nx, ny, nz);
		b.set(-7.5);
		x.set(0);
		for (len_t k = 1; k <= nz; k++)
			for (len_t j = 1; j <= ny; j++)
				for (len_t i = 1; i <= nx; i++) { b(i, j, k) = 3.0 + 1.0 / (1.0 + i + 2.0 * j + 3.0 * k); sb += b(i, j, k); }
		cdr3::solver<cdr3::seven_pt> s(so, conf);
		solve(s, b, x);
		const real_t mb = (real_t)(sb / ((long double)nx * ny * nz));
		for (len_t k = 1; k <= nz; k++)
			for (len_t j = 1; j <= ny; j++)
				for (len_t i = 1; i <= nx; i++) {
					using namespace cedar::cdr3;
					const real_t ax = so(i, j, k, seven_pt::p) * x(i, j, k)
					                  - so(i, j, k, seven_pt::pw) * x(i - 1, j, k) - so(i + 1, j, k, seven_pt::pw) * x(i + 1, j, k)
					                  - so(i, j, k, seven_pt::ps) * x(i, j - 1, k) - so(i, j + 1, k, seven_pt::ps) * x(i, j + 1, k)
					                  - so(i, j, k, seven_pt::b) * x(i, j, k - 1) - so(i, j, k + 1, seven_pt::b) * x(i, j, k + 1);
					const real_t r = (b(i, j, k) - mb) - ax;
					rr += (long double)r * r; bb += (long double)(b(i, j, k) - mb) * (b(i, j, k) - mb); sx += x(i, j, k); sa += std::fabs(x(i, j, k));
				}
		sx /= (long double)nx * ny * nz; sa /= (long double)nx * ny * nz;
	}
	std::printf(", \"mean_x\": %.17g, \"mean_abs_x\": %.17g, \"rel_res\": %.17g}\n", (double)sx, (double)sa,
	            (double)std::sqrt((double)(rr / bb)));
	return 0;
}
